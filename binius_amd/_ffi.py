"""ctypes binding of include/binius_amd.h + Python mirrors of the reference's handle types.

Mirrors (names and argument meaning follow the reference so the parity tests read like
crates/compute_test_utils/src/layer.rs):

  DevSlice        ComputeMemory::FSlice / FSliceMut handle (crates/compute/src/memory.rs:69-234),
                  ALIGNMENT = 1: (device pointer, length); slice / split_at / split_half are O(1)
                  host arithmetic, no device calls.
  BumpAllocator   crates/compute/src/alloc.rs:31-105
  Context         ComputeLayer + ComputeLayerExecutor (crates/compute/src/layer.rs:22, 100)
  KernelExec      recording KernelExecutor (layer.rs:518-590): the kernel-spec closure is run once
                  and its ops are handed to bn_kernel_launch.
"""
import ctypes as C
import os

import numpy as np

BN_OK, BN_ERR_INPUT_VALIDATION, BN_ERR_ALLOC, BN_ERR_DEVICE, BN_ERR_CORE_LIB, BN_ERR_CALLBACK = range(6)
_ERR_NAMES = {1: "InputValidation", 2: "Alloc", 3: "DeviceError", 4: "CoreLibError", 5: "Callback"}

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libbinius_amd.so")
MASK64 = (1 << 64) - 1
ORDER_LOW_TO_HIGH, ORDER_HIGH_TO_LOW = 0, 1  # EvaluationOrder (crates/math/src/fold.rs)
HAL_ML_FOLDED, HAL_ML_TRANSPARENT = 0, 1
NTT_MAX_DIM = 64
BN_ME_MAX_LO_VARS, BN_ME_MAX_JOBS = 10, 4096  # bn_mle_evaluate_batch
BN_MERGE_TILE_LOG2 = 6  # bn_merge_multilins: multilinears of at least twice as many variables are tiled jobs
BN_TOWER_EXPR_MAX_STEPS, BN_TOWER_EXPR_MAX_INPUTS, BN_TOWER_EXPR_MAX_LIVE = 1024, 256, 16  # bn_expr_compile_tower
BN_CC_TOWER_CALLS, BN_CC_TOWER_LAUNCHES, BN_CC_TOWER_BITWISE, BN_CC_TOWER_VALUES, BN_CC_N = 0, 1, 2, 3, 4  # bn_compute_composite_counters
BN_COMPOSE_BATCH_MAX_JOBS, BN_COMPOSE_JOB_DESC_WORDS = 4096, 4  # bn_expr_compile_tower_batch
BN_CCB_CALLS, BN_CCB_LAUNCHES, BN_CCB_JOBS, BN_CCB_PROGRAMS, BN_CCB_N = 0, 1, 2, 3, 4  # bn_compute_composite_batch_counters


def lib_path():
    return _SO


class BnError(RuntimeError):
    """binius_compute::Error (crates/compute/src/layer.rs:706-716)."""

    def __init__(self, code, msg):
        super().__init__("%s: %s" % (_ERR_NAMES.get(code, code), msg))
        self.code = code
        self.kind = _ERR_NAMES.get(code, str(code))


class F128(C.Structure):
    _fields_ = [("lo", C.c_uint64), ("hi", C.c_uint64)]


class Step(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint64), ("cst", F128)]


class MemMap(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("log_min_chunk_size", C.c_uint32),
        ("d_data", C.c_void_p),
        ("len", C.c_uint64),
        ("log_size", C.c_uint32),
    ]


class PeColumn(C.Structure):
    """bn_pe_column: one column of bn_partial_eval_high_batch."""

    _fields_ = [("d_evals", C.c_void_p), ("tower_level", C.c_uint32), ("n_vars", C.c_uint32)]


class PelTerm(C.Structure):
    """bn_pel_term: one constituent column of a job of bn_partial_eval_high_lincomb_batch and its coefficient."""

    _fields_ = [("d_evals", C.c_void_p), ("tower_level", C.c_uint32), ("reserved", C.c_uint32), ("coeff", F128)]


class PelJob(C.Structure):
    """bn_pel_job: one linear combination of bn_partial_eval_high_lincomb_batch, its terms a range of the call's term table."""

    _fields_ = [("n_vars", C.c_uint32), ("first_term", C.c_uint32), ("n_terms", C.c_uint32), ("reserved", C.c_uint32), ("offset", F128)]


PEL_MAX_TERMS = 64  # BN_PEL_MAX_TERMS


class DeriveJob(C.Structure):
    """bn_derive_job: one virtual column of bn_derive_columns_batch."""

    _fields_ = [("kind", C.c_uint32), ("tower_level", C.c_uint32), ("n_vars", C.c_uint32), ("inner_n_vars", C.c_uint32), ("d_inner", C.c_void_p),
                ("d_out", C.c_void_p), ("block_size", C.c_uint32), ("shift_variant", C.c_uint32), ("shift_offset", C.c_uint64), ("start_index", C.c_uint32),
                ("reserved", C.c_uint32), ("nonzero_index", C.c_uint64), ("first_term", C.c_uint32), ("n_terms", C.c_uint32), ("offset", F128)]


DERIVE_SHIFTED, DERIVE_REPEATING, DERIVE_ZERO_PADDED, DERIVE_XOR_COMBINATION = range(4)  # BN_DERIVE_*
SHIFT_CIRCULAR_LEFT, SHIFT_LOGICAL_LEFT, SHIFT_LOGICAL_RIGHT = range(3)  # BN_SHIFT_* (ShiftVariant)


class GenerateJob(C.Structure):
    """bn_generate_job: one generated column of bn_generate_columns_batch."""

    _fields_ = [("kind", C.c_uint32), ("tower_level", C.c_uint32), ("n_vars", C.c_uint32), ("start_index", C.c_uint32), ("d_inner", C.c_void_p),
                ("d_out", C.c_void_p), ("query_size", C.c_uint32), ("reserved", C.c_uint32), ("query_bits", C.c_uint64), ("index", C.c_uint64), ("value", F128)]


GEN_PROJECTED_BITS, GEN_CONSTANT, GEN_STEP_DOWN, GEN_STEP_UP, GEN_SELECT_ROW, GEN_INCREMENTING, GEN_POWERS = range(7)  # BN_GEN_*
GEN_KINDS = {"projected_bits": GEN_PROJECTED_BITS, "constant": GEN_CONSTANT, "step_down": GEN_STEP_DOWN, "step_up": GEN_STEP_UP, "select_row": GEN_SELECT_ROW,
             "incrementing": GEN_INCREMENTING, "powers": GEN_POWERS}


class RsJob(C.Structure):
    """bn_rs_job: one equality indicator of bn_ring_switch_eq_ind_batch."""

    _fields_ = [("d_query", C.c_void_p), ("n_vars", C.c_uint32), ("kappa", C.c_uint32), ("mixing_coeff", F128)]


class FriOracle(C.Structure):
    """bn_fri_oracle: one committed oracle of bn_fri_query_openings."""

    _fields_ = [("d_codeword", C.c_void_p), ("d_nodes", C.c_void_p), ("log_n_cosets", C.c_uint32), ("log_coset_size", C.c_uint32),
                ("layer_depth", C.c_uint32), ("index_shift", C.c_uint32)]


FRI_QUERY_MAX_ORACLES = 32  # BN_FRI_QUERY_MAX_ORACLES


class MePoint(C.Structure):
    """bn_me_point: one point of bn_mle_evaluate_batch, as the tensor expansions of its first lo_vars and its other hi_vars coordinates."""

    _fields_ = [("d_lo", C.c_void_p), ("d_hi", C.c_void_p), ("lo_vars", C.c_uint32), ("hi_vars", C.c_uint32)]


class MeJob(C.Structure):
    """bn_me_job: one column of bn_mle_evaluate_batch and the index of its point."""

    _fields_ = [("d_evals", C.c_void_p), ("tower_level", C.c_uint32), ("n_vars", C.c_uint32), ("point", C.c_uint32), ("reserved", C.c_uint32)]


class HalMultilinear(C.Structure):
    """bn_hal_multilinear: SumcheckMultilinear::{Folded, Transparent} (crates/hal/src/common.rs)."""

    _fields_ = [
        ("kind", C.c_uint32),
        ("tower_level", C.c_uint32),
        ("d_evals", C.c_void_p),
        ("len", C.c_uint64),
        ("suffix_eval", F128),
        ("n_vars_ml", C.c_uint32),
    ]


class HalEvaluator(C.Structure):
    """bn_hal_evaluator: what a SumcheckEvaluator contributes to one round (crates/hal/src/sumcheck_evaluator.rs)."""

    _fields_ = [
        ("composition", C.c_void_p),
        ("composition_at_infinity", C.c_void_p),
        ("eval_point_start", C.c_uint32),
        ("eval_point_end", C.c_uint32),
        ("d_eq_ind", C.c_void_p),
    ]


class KSlice(C.Structure):
    _fields_ = [("buf", C.c_uint32), ("off", C.c_uint64), ("len", C.c_uint64)]


class KOp(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("value", C.c_uint32),
        ("scalar", F128),
        ("expr", C.c_void_p),
        ("n_rows", C.c_uint32),
        ("rows", C.POINTER(KSlice)),
        ("src1", KSlice),
        ("src2", KSlice),
        ("dst", KSlice),
    ]


STEP_KINDS = {"add": 0, "mul": 1, "pow": 2, "const": 3, "var": 4}
MAP_CHUNKED, MAP_CHUNKED_MUT, MAP_LOCAL = range(3)
KOP_DECL_VALUE, KOP_SUM_COMPOSITION, KOP_ADD, KOP_ADD_ASSIGN = range(4)

_lib = None


def lib():
    """Load libbinius_amd.so.  Fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError(
            "binius_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % _SO
        )
    L = C.CDLL(_SO)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    PF = C.POINTER(F128)
    sig = {
        "bn_ctx_create": [i32, u64, C.POINTER(vp)],
        "bn_ctx_destroy": [vp],
        "bn_arena_base": [vp, C.POINTER(vp), C.POINTER(u64)],
        "bn_ctx_set_stream": [vp, vp],
        "bn_sync": [vp],
        "bn_ctx_get_stream": [vp, C.POINTER(vp)],
        "bn_copy_h2d": [vp, vp, u64, vp, u64],
        "bn_copy_d2h": [vp, vp, u64, vp, u64],
        "bn_copy_d2d": [vp, vp, u64, vp, u64],
        "bn_fill": [vp, vp, u64, PF],
        "bn_expr_compile": [vp, C.POINTER(Step), u64, C.POINTER(vp)],
        "bn_expr_free": [vp],
        "bn_expr_n_vars": [vp, C.POINTER(u32)],
        "bn_expr_compile_tower": [vp, C.POINTER(Step), u64, C.POINTER(u32), u32, u32, C.POINTER(vp)],
        "bn_compute_composite_counters": [vp, C.POINTER(u64)],
        "bn_expr_compile_tower_batch": [vp, C.POINTER(vp), u32, C.POINTER(u32), C.POINTER(u64), u32, C.POINTER(vp)],
        "bn_compute_composite_batch_counters": [vp, C.POINTER(u64)],
        "bn_extrapolate_line": [vp, vp, u64, vp, u64, PF],
        "bn_extrapolate_line_batch": [vp, C.POINTER(vp), C.POINTER(vp), u32, u64, PF],
        "bn_extrapolate_line_batch_scaled": [vp, C.POINTER(vp), C.POINTER(vp), u32, u64, PF, u32, PF],
        "bn_tensor_expand": [vp, vp, u64, u32, PF, u32],
        "bn_inner_product": [vp, vp, u64, u32, vp, u64, PF],
        "bn_fold_left": [vp, vp, u64, u32, vp, u64, vp, u64],
        "bn_fold_right": [vp, vp, u64, u32, vp, u64, vp, u64],
        "bn_fri_fold": [vp, C.POINTER(u64), u32, u32, u32, u32, PF, u32, vp, u64, vp, u64],
        "bn_compute_composite": [vp, C.POINTER(vp), u32, u64, vp, u64, vp],
        "bn_pairwise_product_reduce": [vp, vp, u64, C.POINTER(vp), C.POINTER(u64), u32],
        "bn_product_tree_layers": [vp, u32, C.POINTER(u32), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), PF],
        "bn_pad_with_ones": [vp, u32, C.POINTER(u32), C.POINTER(vp), C.POINTER(u64), C.POINTER(vp)],
        "bn_exp_circuit_layers": [vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(vp), PF, C.POINTER(vp), C.POINTER(vp)],
        "bn_bits_to_b128": [vp, u32, C.POINTER(u32), C.POINTER(vp), C.POINTER(vp)],
        "bn_exp_counters": [vp, C.POINTER(u64)],
        "bn_flush_witness_batch": [vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(vp), C.POINTER(u32), C.POINTER(vp), C.POINTER(u32), PF, PF,
                                   C.POINTER(vp), C.POINTER(u64)],
        "bn_flush_counters": [vp, C.POINTER(u64)],
        "bn_partial_eval_high_batch": [vp, vp, u32, vp, u32, C.POINTER(vp)],
        "bn_partial_eval_counters": [vp, C.POINTER(u64)],
        "bn_partial_eval_high_lincomb_batch": [vp, vp, u32, vp, u32, vp, u32, C.POINTER(vp)],
        "bn_partial_eval_lincomb_counters": [vp, C.POINTER(u64)],
        "bn_univariate_fold_batch": [vp, vp, u32, u32, PF, C.POINTER(vp)],
        "bn_univariate_fold_counters": [vp, C.POINTER(u64)],
        "bn_ring_switch_eq_ind_batch": [vp, vp, u32, PF, u32, C.POINTER(vp)],
        "bn_ring_switch_counters": [vp, C.POINTER(u64)],
        "bn_mle_evaluate_batch": [vp, vp, u32, vp, u32, PF],
        "bn_mle_evaluate_counters": [vp, C.POINTER(u64)],
        "bn_merge_multilins": [vp, u32, C.POINTER(u32), C.POINTER(vp), vp, u32, u32],
        "bn_merge_counters": [vp, C.POINTER(u64)],
        "bn_derive_columns_batch": [vp, vp, u32, C.POINTER(vp), u32],
        "bn_derive_counters": [vp, C.POINTER(u64)],
        "bn_generate_columns_batch": [vp, vp, u32],
        "bn_generate_counters": [vp, C.POINTER(u64)],
        "bn_fri_query_proof_elems": [vp, u32, u64, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)],
        "bn_fri_query_openings": [vp, vp, u32, vp, u64, C.POINTER(u64), u64, u32, vp, u64],
        "bn_fri_query_counters": [vp, C.POINTER(u64)],
        "bn_log_chunks_range": [C.POINTER(MemMap), u32, C.POINTER(u32), C.POINTER(u32)],
        "bn_pick_log_chunks": [C.POINTER(MemMap), u32, C.POINTER(u32)],
        "bn_kernel_launch": [vp, C.POINTER(MemMap), u32, C.POINTER(KOp), u32, C.POINTER(u32), u32, u32, PF, vp],
        "bn_hal_round_evals": [vp, u32, u32, vp, u32, C.POINTER(HalMultilinear), u32, C.POINTER(HalEvaluator), u32, PF, u32, PF],
        "bn_hal_fold_multilinear": [vp, u32, u32, C.POINTER(HalMultilinear), PF, vp, u32, vp, u64, C.POINTER(u64)],
        "bn_zerocheck_univariate_evals": [vp, u32, u32, C.POINTER(HalMultilinear), u32, C.POINTER(Step), C.POINTER(u32), C.POINTER(u32), u32, vp, u64, u32, PF, PF],
        "bn_zerocheck_univariate_evals_base": [vp, u32, u32, u32, C.POINTER(HalMultilinear), u32, C.POINTER(Step), C.POINTER(u32), C.POINTER(u32), u32, vp, u64, u32, PF, PF],
        "bn_ntt_forward": [vp, vp, u32, u32, C.POINTER(u64), u32, u32, u32, u32, u64, u32, u32],
        "bn_ntt_inverse": [vp, vp, u32, u32, C.POINTER(u64), u32, u32, u32, u32, u64, u32, u32],
        "bn_ntt_s_evals": [u32, u32, C.POINTER(u64)],
        "bn_scalar_mul": [PF, PF, PF],
        "bn_scalar_invert": [PF, PF],
        "bn_prof_begin": [vp],
        "bn_prof_end": [vp, C.POINTER(C.c_double), C.POINTER(u64)],
        "bn_arm_counters": [vp, C.POINTER(u64)],
        "bn_group_counters": [vp, C.POINTER(u64)],
        "bn_fp4_last_grids": [vp, C.POINTER(u64)],
        "bn_ntt_counters": [vp, C.POINTER(u64)],
        "bn_fri_counters": [vp, C.POINTER(u64)],
        "bn_fold_counters": [vp, C.POINTER(u64)],
        "bn_inner_product_counters": [vp, C.POINTER(u64)],
        "bn_hal_counters": [vp, C.POINTER(u64)],
        "bn_xor_reduce": [vp, vp, u32, u32, PF],
        "bn_host_scratch": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)],
        "bn_device_numa_node": [C.c_int, C.POINTER(C.c_int)],
        "bn_merkle_build": [vp, vp, u64, u64, vp],
        "bn_groestl256_leaves": [vp, vp, u64, u64, vp],
        "bn_groestl256_compress_layer": [vp, vp, u64, vp],
        "bn_gather_d2h": [vp, vp, C.POINTER(u64), u64, u64, vp],
        "bn_timer_begin": [vp],
        "bn_timer_end_ms": [vp, C.POINTER(C.c_float)],
        "bn_peer_create": [vp, u32, u32, C.c_char_p],
        "bn_peer_connect": [vp, C.c_char_p],
        "bn_peer_set_active": [vp, C.c_int],
        "bn_peer_stats": [vp, C.POINTER(u64)],
        "bn_host_tail_allow_peer": [vp, C.c_int],
        "bn_host_tail_active": [vp, C.POINTER(C.c_int)],
        "bn_peer_destroy": [vp],
    }
    for name, args in sig.items():
        fn = getattr(L, name)  # AttributeError here == the .so does not export a declared symbol
        fn.argtypes = args
        fn.restype = C.c_int
    L.bn_last_error.restype = C.c_char_p
    L.bn_version.restype = C.c_char_p
    _lib = L
    return L


ABI_SYMBOLS = [
    "bn_last_error", "bn_version", "bn_ctx_create", "bn_ctx_destroy", "bn_arena_base", "bn_ctx_set_stream", "bn_sync", "bn_ctx_get_stream",
    "bn_copy_h2d", "bn_copy_d2h", "bn_copy_d2d", "bn_fill", "bn_expr_compile", "bn_expr_free", "bn_expr_n_vars",
    "bn_extrapolate_line", "bn_extrapolate_line_batch", "bn_tensor_expand", "bn_inner_product", "bn_fold_left", "bn_fold_right", "bn_fri_fold",
    "bn_compute_composite", "bn_pairwise_product_reduce", "bn_log_chunks_range", "bn_pick_log_chunks",
    "bn_kernel_launch", "bn_ntt_forward", "bn_ntt_inverse", "bn_ntt_s_evals", "bn_scalar_mul", "bn_scalar_invert",
    "bn_timer_begin", "bn_timer_end_ms", "bn_prof_begin", "bn_prof_end", "bn_arm_counters", "bn_group_counters", "bn_fp4_last_grids", "bn_ntt_counters", "bn_fri_counters", "bn_fold_counters", "bn_inner_product_counters", "bn_hal_counters", "bn_xor_reduce", "bn_host_scratch", "bn_device_numa_node",
    "bn_merkle_build", "bn_groestl256_leaves", "bn_groestl256_compress_layer", "bn_gather_d2h",
    "bn_hal_round_evals", "bn_hal_fold_multilinear", "bn_extrapolate_line_batch_scaled", "bn_zerocheck_univariate_evals", "bn_zerocheck_univariate_evals_base",
    "bn_product_tree_layers", "bn_pad_with_ones", "bn_exp_circuit_layers", "bn_bits_to_b128", "bn_exp_counters",
    "bn_partial_eval_high_batch", "bn_partial_eval_counters", "bn_flush_witness_batch", "bn_flush_counters",
    "bn_univariate_fold_batch", "bn_univariate_fold_counters", "bn_ring_switch_eq_ind_batch", "bn_ring_switch_counters",
    "bn_mle_evaluate_batch", "bn_mle_evaluate_counters", "bn_partial_eval_high_lincomb_batch", "bn_partial_eval_lincomb_counters",
    "bn_merge_multilins", "bn_merge_counters", "bn_derive_columns_batch", "bn_derive_counters", "bn_generate_columns_batch", "bn_generate_counters", "bn_expr_compile_tower", "bn_compute_composite_counters", "bn_expr_compile_tower_batch", "bn_compute_composite_batch_counters", "bn_fri_query_proof_elems", "bn_fri_query_openings", "bn_fri_query_counters",
    "bn_peer_create", "bn_peer_connect", "bn_peer_set_active", "bn_peer_stats", "bn_peer_destroy", "bn_host_tail_allow_peer", "bn_host_tail_active",
]


def _check(rc):
    if rc != BN_OK:
        raise BnError(rc, lib().bn_last_error().decode())


def fri_oracle_table(oracles):
    """The bn_fri_oracle array of tuples (codeword, nodes, log_n_cosets, log_coset_size, layer_depth, index_shift); codeword and nodes
    are DevSlices or None (bn_fri_query_proof_elems reads the sizes only)."""
    return (FriOracle * max(1, len(oracles)))(*[FriOracle(o[0].ptr if o[0] is not None else None, o[1].ptr if o[1] is not None else None, o[2], o[3], o[4], o[5])
                                                for o in oracles])


def fri_query_proof_elems(oracles, terminate_elems, n_queries):
    """bn_fri_query_proof_elems: (header, per-query record, total) of the block bn_fri_query_openings writes, in field elements.  Pure
    host arithmetic: no context, no device."""
    h, r, t = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(lib().bn_fri_query_proof_elems(C.cast(fri_oracle_table(oracles), C.c_void_p), len(oracles), terminate_elems, n_queries, C.byref(h), C.byref(r), C.byref(t)))
    return h.value, r.value, t.value


def device_numa_node(device=0):
    """NUMA node of the host the device hangs off, or None if the platform does not say (bn_device_numa_node)."""
    node = C.c_int(-1)
    _check(lib().bn_device_numa_node(int(device), C.byref(node)))
    return node.value if node.value >= 0 else None


def bind_host_thread_to_device(device=0):
    """Restrict the calling thread to the CPUs of the device's NUMA node (what `numactl --cpunodebind` does): every small
    sumcheck round is a host -> device -> host round trip, and from the other socket of a 2-socket host each one also
    crosses the socket interconnect (15.0 -> 17.1 us per two-round launch measured).  Returns a description of what was
    done; never widens the current affinity, does nothing when the node or its CPU list is unknown."""
    import os

    try:
        node = device_numa_node(device)
    except Exception as ex:  # (a measurement convenience must never be the reason a run fails)
        return "unchanged (%s)" % type(ex).__name__
    if node is None or not hasattr(os, "sched_setaffinity"):
        return "unchanged (no NUMA information for the device)"
    try:
        txt = open("/sys/devices/system/node/node%d/cpulist" % node).read().strip()
    except OSError:
        return "unchanged (node %d has no cpulist)" % node
    cpus = set()
    try:
        for part in txt.split(","):
            if "-" in part:
                a, b = part.split("-")
                cpus.update(range(int(a), int(b) + 1))
            elif part:
                cpus.add(int(part))
    except ValueError:
        return "unchanged (unreadable cpulist of node %d)" % node
    try:
        want = cpus & os.sched_getaffinity(0)
        if not want:
            return "unchanged (none of node %d's CPUs are allowed to this process)" % node
        os.sched_setaffinity(0, want)
    except OSError as ex:
        return "unchanged (sched_setaffinity: %s)" % ex
    return "NUMA node %d (%d CPUs)" % (node, len(want))


def to_f128(x):
    x = int(x)
    return F128(x & MASK64, (x >> 64) & MASK64)


def from_f128(f):
    return int(f.lo) | (int(f.hi) << 64)


def _f128_array(vals):
    arr = (F128 * max(1, len(vals)))()
    for i, v in enumerate(vals):
        arr[i] = to_f128(v)
    return arr


def make_steps(steps):
    out = (Step * max(1, len(steps)))()
    for i, s in enumerate(steps):
        k = STEP_KINDS[s[0]]
        out[i].kind = k
        if k in (0, 1, 2):
            out[i].a, out[i].b = s[1], s[2]
        elif k == 3:
            out[i].cst = to_f128(s[1])
        else:
            out[i].a = s[1]
    return out


class HostField:
    """O(1)-per-round protocol scalars on the host (bn_scalar_mul / bn_scalar_invert)."""

    @staticmethod
    def mul(a, b):
        x, y, o = to_f128(a), to_f128(b), F128()
        _check(lib().bn_scalar_mul(C.byref(x), C.byref(y), C.byref(o)))
        return from_f128(o)

    @staticmethod
    def invert(a):
        x, o = to_f128(a), F128()
        _check(lib().bn_scalar_invert(C.byref(x), C.byref(o)))
        return from_f128(o)


# ------------------------------------------------------------------ memory handles
class DevSlice:
    """Opaque handle to a slice of F in device memory: (pointer, len).  ALIGNMENT = 1."""

    ALIGNMENT = 1
    __slots__ = ("ptr", "len")

    def __init__(self, ptr, length):
        self.ptr = int(ptr)
        self.len = int(length)

    def __len__(self):
        return self.len

    def __repr__(self):
        return "DevSlice(0x%x, len=%d)" % (self.ptr, self.len)

    def slice(self, start=0, end=None):
        end = self.len if end is None else end
        assert 0 <= start <= end <= self.len, "slice out of range"
        return DevSlice(self.ptr + 16 * start, end - start)

    def split_at(self, mid):
        return self.slice(0, mid), self.slice(mid, self.len)

    def split_half(self):
        assert self.len > 1 and (self.len & (self.len - 1)) == 0, "data length must be a power of two greater than 1"
        return self.split_at(self.len // 2)

    def chunks(self, chunk_len):
        assert self.len % chunk_len == 0
        return [self.slice(i, i + chunk_len) for i in range(0, self.len, chunk_len)]


class BumpAllocator:
    """crates/compute/src/alloc.rs:31-105 over a DevSlice (or another allocator's remainder)."""

    def __init__(self, buffer):
        self._buf = buffer

    def alloc(self, n):
        if self._buf.len < n:
            raise BnError(BN_ERR_ALLOC, "allocator is out of memory")
        lhs, rhs = self._buf.split_at(n)
        self._buf = rhs
        return lhs

    def capacity(self):
        return self._buf.len

    def subscope_allocator(self):
        return BumpAllocator(self._buf.slice())


class Expr:
    """ExprEval: handle returned by compile_expr (layer.rs:57)."""

    def __init__(self, handle, steps):
        self.handle = handle
        self.steps = list(steps)

    def n_vars(self):
        n = C.c_uint32()
        _check(lib().bn_expr_n_vars(self.handle, C.byref(n)))
        return n.value

    def free(self):
        if self.handle:
            lib().bn_expr_free(self.handle)
            self.handle = None


# ------------------------------------------------------------------ recording KernelExecutor
class KernelBuffer:
    """KernelBuffer::{Ref,Mut} (layer.rs:682-704): a chunk-relative view of mapped buffer `buf`."""

    __slots__ = ("buf", "off", "len", "mutable")

    def __init__(self, buf, off, length, mutable):
        self.buf, self.off, self.len, self.mutable = buf, off, length, mutable

    def __len__(self):
        return self.len

    def to_ref(self):
        return KernelBuffer(self.buf, self.off, self.len, False)

    def slice(self, start=0, end=None):
        end = self.len if end is None else end
        assert 0 <= start <= end <= self.len
        return KernelBuffer(self.buf, self.off + start, end - start, self.mutable)

    def triple(self):
        return (self.buf, self.off, self.len)


class KernelValue:
    __slots__ = ("id",)

    def __init__(self, vid):
        self.id = vid


class KernelExec:
    """Recording KernelExecutor: collects the ops the kernel-spec closure issues."""

    def __init__(self):
        self.ops = []
        self.n_values = 0

    def decl_value(self, init):
        v = KernelValue(self.n_values)
        self.n_values += 1
        self.ops.append({"op": "decl", "value": v.id, "init": int(init)})
        return v

    def sum_composition_evals(self, inputs, composition, batch_coeff, accumulator):
        row_len = len(inputs[0]) if inputs else 0
        for r in inputs:
            assert len(r) == row_len  # SlicesBatch::new (memory.rs:39-45)
        self.ops.append(
            {"op": "sum", "value": accumulator.id, "expr": composition, "coeff": int(batch_coeff), "rows": [r.triple() for r in inputs]}
        )

    def add(self, log_len, src1, src2, dst):
        assert len(src1) == 1 << log_len and len(src2) == 1 << log_len and len(dst) == 1 << log_len
        assert dst.mutable
        self.ops.append({"op": "add", "src1": src1.triple(), "src2": src2.triple(), "dst": dst.triple()})

    def add_assign(self, log_len, src, dst):
        assert len(src) == 1 << log_len and len(dst) == 1 << log_len
        assert dst.mutable
        self.ops.append({"op": "add_assign", "src": src.triple(), "dst": dst.triple()})


def _make_maps(mem_maps):
    mm = (MemMap * max(1, len(mem_maps)))()
    for i, m in enumerate(mem_maps):
        if m[0] == "local":
            mm[i].kind = MAP_LOCAL
            mm[i].log_size = m[1]
        else:
            mm[i].kind = MAP_CHUNKED if m[0] == "chunked" else MAP_CHUNKED_MUT
            mm[i].d_data = m[1].ptr
            mm[i].len = m[1].len
            mm[i].log_min_chunk_size = m[2]
    return mm


def log_chunks_range(mem_maps):
    """KernelMemMap::log_chunks_range (layer.rs:617-644). Host only."""
    mm = _make_maps(mem_maps)
    s, e = C.c_uint32(), C.c_uint32()
    _check(lib().bn_log_chunks_range(mm, len(mem_maps), C.byref(s), C.byref(e)))
    return range(s.value, e.value)


def ntt_s_evals(tw_level, log_domain):
    """OnTheFlyTwiddleAccess::generate for the canonical subspace. Host only."""
    s = np.zeros(NTT_MAX_DIM * NTT_MAX_DIM, dtype=np.uint64)
    _check(lib().bn_ntt_s_evals(tw_level, log_domain, s.ctypes.data_as(C.POINTER(C.c_uint64))))
    return s


# ------------------------------------------------------------------ the layer
class Context:
    """ComputeLayer + executor over one GPU.  `arena_elems` F elements of device memory are
    allocated up front (like FastCpuLayerHolder::new(host, dev)); `dev_alloc()` bump-allocates."""

    def __init__(self, device=0, arena_elems=0):
        self._h = C.c_void_p()
        _check(lib().bn_ctx_create(device, arena_elems, C.byref(self._h)))
        self.device = device
        base, n = C.c_void_p(), C.c_uint64()
        _check(lib().bn_arena_base(self._h, C.byref(base), C.byref(n)))
        self.arena = DevSlice(base.value or 0, n.value)
        self._exprs = []

    def close(self):
        if self._h:
            for e in self._exprs:
                e.free()
            lib().bn_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def dev_alloc(self):
        return BumpAllocator(self.arena.slice())

    def set_stream(self, hip_stream):
        _check(lib().bn_ctx_set_stream(self._h, hip_stream))

    def get_stream(self):
        """The stream the context runs on, as an integer handle; everything deferred is launched first (bn_ctx_get_stream)."""
        s = C.c_void_p()
        _check(lib().bn_ctx_get_stream(self._h, C.byref(s)))
        return s.value or 0

    def sync(self):
        _check(lib().bn_sync(self._h))

    def timer_begin(self):
        _check(lib().bn_timer_begin(self._h))

    def timer_end_ms(self):
        ms = C.c_float()
        _check(lib().bn_timer_end_ms(self._h, C.byref(ms)))
        return ms.value

    PROF_CLASSES = ("round_eval", "fold", "tensor_expand", "ntt", "other", "fold_eval", "tail", "fold_eval_small", "fold_eval_mfma", "round_eval_mfma",
                    "fold_eval8")

    def prof_begin(self):
        _check(lib().bn_prof_begin(self._h))

    def prof_end(self):
        ms = (C.c_double * len(self.PROF_CLASSES))()
        cnt = (C.c_uint64 * len(self.PROF_CLASSES))()
        _check(lib().bn_prof_end(self._h, ms, cnt))
        return {k: (ms[i], int(cnt[i])) for i, k in enumerate(self.PROF_CLASSES)}

    def arm_counters(self):
        """Armed rounds (csrc/arm.hpp): {hits, cancels, expired} since the context was created; two-round launches
        (csrc/kernels_foldeval8.hip): their number and the rounds the host answered from their precomputed sums."""
        c = (C.c_uint64 * 15)()
        _check(lib().bn_arm_counters(self._h, c))
        return {"hits": int(c[0]), "cancels": int(c[1]), "expired": int(c[2]), "ns_wait": int(c[3]), "ns_launch": int(c[4]), "ns_parse": int(c[5]),
                "hosted": int(c[6]), "two_round": int(c[7]), "shadow_created": int(c[8]), "shadow_rounds": int(c[9]), "shadow_dropped": int(c[10]),
                # host tail (abi_kernels.cpp): instances the host took over, round evaluations it answered, fold chains launched
                "ht_started": int(c[11]), "ht_rounds": int(c[12]), "ht_flushed": int(c[13]), "ht_max": int(c[14])}

    def group_counters(self):
        """Claim groups (csrc/abi_group.cpp): how the call shape of piop::prove -- k product claims over m multilinears per
        prover, several provers front-loaded on one layer -- was run: launches of the group kernel, claims evaluated fused
        with their folds / on pre-folded arrays, plain fold launches of a round, claims of other provers carried along,
        execute() calls answered from sums computed ahead, execute() calls on this path, deferred folds forced out."""
        c = (C.c_uint64 * 14)()
        _check(lib().bn_group_counters(self._h, c))
        keys = ("launches", "jobs_fused", "jobs_eval", "prefolds", "spec_jobs", "spec_hits", "evals", "flushed_folds", "hosted_started", "hosted_evals",
                "hosted_folds", "hosted_writebacks", "jobs_fold", "chains")
        return {k: int(c[i]) for i, k in enumerate(keys)}

    def fp4_last_grids(self):
        """How the last FP4 round evaluation and the last fused FP4 fold + evaluation of this process were launched
        (bn_fp4_last_grids): workgroups, most tiles per workgroup, whether the round evaluation ran its stager / Gram wave form, and the largest
        share of a workgroup in any such launch of the process so far."""
        c = (C.c_uint64 * 7)()
        _check(lib().bn_fp4_last_grids(self._h, c))
        return {"re_grid": int(c[0]), "re_tiles": int(c[1]), "re_ws": int(c[2]), "fe_grid": int(c[3]), "fe_tiles": int(c[4]),
                "re_max_tiles": int(c[5]), "fe_max_tiles": int(c[6])}

    def ntt_counters(self):
        """bn_ntt_forward / bn_ntt_inverse calls of this context served by each kernel family (bn_ntt_counters): the bit-sliced
        kernels, the LDS-tiled kernel, the per-layer kernel.  Rejected calls and accepted no-ops count nowhere."""
        c = (C.c_uint64 * 3)()
        _check(lib().bn_ntt_counters(self._h, c))
        return {"bs": int(c[0]), "tiled": int(c[1]), "layer": int(c[2])}

    def fri_counters(self):
        """Passes launched by the bn_fri_fold calls of this context, by form (bn_fri_counters): one challenge per pass, two / three
        interleave challenges in one pass, two / three challenges with a butterfly level among them in one pass (ntt3: a measurement
        form, 0 in the normal build), and the calls without a challenge (one copy each).  Rejected calls count nowhere."""
        c = (C.c_uint64 * 6)()
        _check(lib().bn_fri_counters(self._h, c))
        return {k: int(c[i]) for i, k in enumerate(("one", "inter2", "inter3", "ntt2", "ntt3", "copies"))}

    FOLD_COUNTERS = ("right_mfma", "right_tab", "right_scalar", "left_pe", "left_mfma", "left_tab", "left_scalar", "ring2", "ring4", "ring8",
                     "ring_left2", "ring_left4", "ring_left8", "last_grid", "last_prep", "n_cu")

    def fold_counters(self):
        """Which kernel answered the bn_fold_right / bn_fold_left calls of this context (bn_fold_counters).  Every accepted call counts
        in exactly one of right_mfma / right_tab / right_scalar (the matrix cores, the nibble tables, the scalar kernel), left_pe (handed
        to the partial-evaluation kernel), left_mfma / left_tab / left_scalar; ring<R> / ring_left<R> split the matrix-core calls by
        kernel instantiation; last_grid / last_prep are the workgroups of the last matrix-core launch and the tower level of its table
        preparation, n_cu the compute units of the device, by which the launchers size their grids.  Rejected calls move nothing."""
        c = (C.c_uint64 * len(self.FOLD_COUNTERS))()
        _check(lib().bn_fold_counters(self._h, c))
        return {k: int(c[i]) for i, k in enumerate(self.FOLD_COUNTERS)}

    def inner_product_counters(self):
        """Which kernel answered the bn_inner_product calls of this context (bn_inner_product_counters): the F x F split sum on the
        matrix cores, the 9-lane split kernel, the bit-sliced B32 kernel (k_ip32), the scalar kernel (k_inner_product).  Rejected
        calls count nowhere."""
        c = (C.c_uint64 * 4)()
        _check(lib().bn_inner_product_counters(self._h, c))
        return {k: int(c[i]) for i, k in enumerate(("mfma_split", "split9", "ip32", "scalar"))}

    HAL_COUNTERS = ("coef", "eq_set", "in_parts", "monomials", "rows_batched", "rows_per_point", "interpreter", "mono_strided", "mono_product2",
                    "mono_product3", "mono_xor_sum", "mono_const", "rows_launches", "rows_written", "rows_in_place", "transparent", "n_cu")

    def hal_counters(self):
        """Which route answered the bn_hal_round_evals calls of this context (bn_hal_counters): every request answered with BN_OK that
        asked for a value counts in exactly one of coef / eq_set / in_parts / monomials / rows_batched / rows_per_point / interpreter (the
        parts of a request counted under in_parts come back through the entry point and count again, under their own routes).  mono_*:
        the monomial route's jobs by kind (the strided matrix-core launch of Low-to-High pairs, the product-sum kernels over two / three
        factors, launches of the lone column's streaming sum, constants skipped); rows_launches / rows_written / rows_in_place: launches
        of the rows kernel, the rows they wrote, the halves read where they lie; transparent: multilinears partially evaluated into
        scratch; n_cu: the compute units of the device.  A call that returns an error moves nothing."""
        c = (C.c_uint64 * len(self.HAL_COUNTERS))()
        _check(lib().bn_hal_counters(self._h, c))
        return {k: int(c[i]) for i, k in enumerate(self.HAL_COUNTERS)}

    # ---- ComputeLayer
    def copy_h2d(self, src, dst):
        """src: numpy uint64 array of shape (n, 2)."""
        src = np.ascontiguousarray(src, dtype=np.uint64).reshape(-1, 2)
        _check(lib().bn_copy_h2d(self._h, src.ctypes.data, src.shape[0], dst.ptr, dst.len))

    def copy_d2h(self, src, dst=None):
        if dst is None:
            dst = np.zeros((src.len, 2), dtype=np.uint64)
        assert dst.dtype == np.uint64 and dst.flags["C_CONTIGUOUS"]
        _check(lib().bn_copy_d2h(self._h, src.ptr, src.len, dst.ctypes.data, dst.reshape(-1, 2).shape[0]))
        return dst

    def copy_d2d(self, src, dst):
        _check(lib().bn_copy_d2d(self._h, src.ptr, src.len, dst.ptr, dst.len))

    def fill(self, slice_, value):
        v = to_f128(value)
        _check(lib().bn_fill(self._h, slice_.ptr, slice_.len, C.byref(v)))

    def compile_expr(self, steps):
        st = make_steps(steps)
        h = C.c_void_p()
        _check(lib().bn_expr_compile(self._h, st, len(steps), C.byref(h)))
        e = Expr(h, steps)
        self._exprs.append(e)
        return e

    def expr_compile_tower(self, steps, input_levels, out_level):
        """bn_expr_compile_tower: a tower-typed expression for compute_composite_tower.  steps as for compile_expr; input_levels[v] is
        the tower level (0 or 3 .. 7) at which input v is packed, out_level the output's.  Every other consumer of an Expr rejects it."""
        st = make_steps(steps)
        lv = (C.c_uint32 * max(1, len(input_levels)))(*input_levels)
        h = C.c_void_p()
        _check(lib().bn_expr_compile_tower(self._h, st, len(steps), lv, len(input_levels), out_level, C.byref(h)))
        e = Expr(h, steps)
        e.input_levels, e.out_level = list(input_levels), out_level
        self._exprs.append(e)
        return e

    def expr_compile_tower_batch(self, exprs, jobs):
        """bn_expr_compile_tower_batch: one handle for a batch of expr_compile_tower expressions, for compute_composite_tower_batch.
        jobs: (expr index, first_row, n_vars, out_offset) each, or a 5-tuple with `reserved` last.  The batch copies the members'
        programs: they may be freed right after."""
        hs = (C.c_void_p * max(1, len(exprs)))(*[e.handle for e in exprs])
        desc = (C.c_uint32 * max(4, 4 * len(jobs)))()
        offs = (C.c_uint64 * max(1, len(jobs)))()
        for i, j in enumerate(jobs):
            desc[4 * i : 4 * i + 4] = [j[0], j[1], j[2], j[4] if len(j) > 4 else 0]
            offs[i] = j[3]
        h = C.c_void_p()
        _check(lib().bn_expr_compile_tower_batch(self._h, hs, len(exprs), desc, offs, len(jobs), C.byref(h)))
        e = Expr(h, [])
        self._exprs.append(e)
        return e

    def compute_composite_batch_counters(self):
        """bn_compute_composite_batch_counters: accepted compute_composite calls with a batch, their launches, the jobs they served, the
        distinct programs they uploaded.  Rejected calls count nowhere."""
        c = (C.c_uint64 * BN_CCB_N)()
        _check(lib().bn_compute_composite_batch_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "jobs": int(c[2]), "programs": int(c[3])}

    def compute_composite_counters(self):
        """bn_compute_composite_counters: accepted compute_composite calls with a tower-typed expression, their launches, how many ran
        at level 0 (bitwise) and at levels 3 .. 7 (per value).  Rejected calls count nowhere."""
        c = (C.c_uint64 * 4)()
        _check(lib().bn_compute_composite_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "bitwise": int(c[2]), "values": int(c[3])}

    # ---- ComputeLayerExecutor
    def extrapolate_line(self, evals_0, evals_1, z):
        zz = to_f128(z)
        _check(lib().bn_extrapolate_line(self._h, evals_0.ptr, evals_0.len, evals_1.ptr, evals_1.len, C.byref(zz)))

    def extrapolate_line_batch(self, evals_0, evals_1, z):
        """The `map` scope of a fold (v3/bivariate_product.rs:217-228): the same z applied to several
        (evals_0, evals_1) pairs of equal length."""
        n = evals_0[0].len if evals_0 else 0
        for a, b in zip(evals_0, evals_1):
            if a.len != n or b.len != n:
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: extrapolate_line batch slices differ in length")
        p0 = (C.c_void_p * len(evals_0))(*[a.ptr for a in evals_0])
        p1 = (C.c_void_p * len(evals_1))(*[b.ptr for b in evals_1])
        zz = to_f128(z)
        _check(lib().bn_extrapolate_line_batch(self._h, p0, p1, len(evals_0), n, C.byref(zz)))

    def extrapolate_line_batch_scaled(self, evals_0, evals_1, z, scale_mask, hi_scale):
        """Extension: the batch fold, then the upper half of every folded array whose bit is set times hi_scale."""
        n = evals_0[0].len
        p0 = (C.c_void_p * len(evals_0))(*[a.ptr for a in evals_0])
        p1 = (C.c_void_p * len(evals_1))(*[b.ptr for b in evals_1])
        zz, hs = to_f128(z), to_f128(hi_scale)
        _check(lib().bn_extrapolate_line_batch_scaled(self._h, p0, p1, len(evals_0), n, C.byref(zz), scale_mask, C.byref(hs)))

    def tensor_expand(self, log_n, coordinates, data):
        c = _f128_array(list(coordinates))
        _check(lib().bn_tensor_expand(self._h, data.ptr, data.len, log_n, c, len(coordinates)))

    def inner_product(self, a_in, tower_level, b_in):
        out = F128()
        _check(lib().bn_inner_product(self._h, a_in.ptr, a_in.len, tower_level, b_in.ptr, b_in.len, C.byref(out)))
        return from_f128(out)

    def fold_left(self, mat, tower_level, vec, out):
        _check(lib().bn_fold_left(self._h, mat.ptr, mat.len, tower_level, vec.ptr, vec.len, out.ptr, out.len))

    def fold_right(self, mat, tower_level, vec, out):
        _check(lib().bn_fold_right(self._h, mat.ptr, mat.len, tower_level, vec.ptr, vec.len, out.ptr, out.len))

    # ---- the old HAL (binius_hal::ComputationBackend, crates/hal/src/backend.rs:35-84) on device-resident multilinears
    @staticmethod
    def _hal_ml(ml):
        """ml: ('folded', DevSlice, suffix_eval) | ('transparent', DevSlice of packed values, tower_level, n_vars_ml)."""
        m = HalMultilinear()
        if ml[0] == "folded":
            m.kind, m.d_evals, m.len, m.suffix_eval = HAL_ML_FOLDED, ml[1].ptr, ml[1].len, to_f128(ml[2])
        else:
            m.kind, m.d_evals, m.len, m.tower_level, m.n_vars_ml = HAL_ML_TRANSPARENT, ml[1].ptr, ml[1].len, ml[2], ml[3]
        return m

    def hal_round_evals(self, order, n_vars, tensor_query, multilinears, evaluators, nontrivial_points):
        """sumcheck_compute_round_evals (backend.rs:52-67).  evaluators: dicts {composition: Expr, composition_at_infinity:
        Expr, start, end, eq_ind: DevSlice | None}; tensor_query: DevSlice of the query expansion or None.  Returns one list
        of values per evaluator (its evaluation point indices start..end)."""
        mls = (HalMultilinear * max(1, len(multilinears)))(*[self._hal_ml(m) for m in multilinears])
        evs = (HalEvaluator * max(1, len(evaluators)))()
        total = 0
        for k, e in enumerate(evaluators):
            evs[k].composition = e["composition"].handle
            evs[k].composition_at_infinity = e["composition_at_infinity"].handle
            evs[k].eval_point_start, evs[k].eval_point_end = e["start"], e["end"]
            evs[k].d_eq_ind = e["eq_ind"].ptr if e.get("eq_ind") is not None else None
            total += max(0, e["end"] - e["start"])
        pts = _f128_array(list(nontrivial_points))
        out = (F128 * max(1, total))()
        q_ptr = tensor_query.ptr if tensor_query is not None else None
        q_vars = (tensor_query.len.bit_length() - 1) if tensor_query is not None else 0
        _check(lib().bn_hal_round_evals(self._h, order, n_vars, q_ptr, q_vars, mls, len(multilinears), evs, len(evaluators), pts,
                                        len(nontrivial_points), out))
        res, off = [], 0
        for e in evaluators:
            cnt = max(0, e["end"] - e["start"])
            res.append([from_f128(out[off + t]) for t in range(cnt)])
            off += cnt
        return res

    def hal_fold_multilinear(self, order, n_vars, multilinear, challenge, tensor_query, out):
        """One multilinear of sumcheck_fold_multilinears (backend.rs:69-78): returns the number of evaluations written."""
        m = self._hal_ml(multilinear)
        z = to_f128(challenge)
        n = C.c_uint64()
        q_ptr = tensor_query.ptr if tensor_query is not None else None
        q_vars = (tensor_query.len.bit_length() - 1) if tensor_query is not None else 0
        _check(lib().bn_hal_fold_multilinear(self._h, order, n_vars, C.byref(m), C.byref(z), q_ptr, q_vars, out.ptr, out.len, C.byref(n)))
        return n.value

    def zerocheck_univariate_evals_base(self, base_level, n_vars, skip_rounds, columns, compositions, degrees, eq, max_domain_size, batch_coeff=None):
        """zerocheck_univariate_evals for every arm of constraint_system/prove.rs:483-490 (bn_zerocheck_univariate_evals_base):
        base_level 3 .. 7 = compositions over B8 .. B128, columns at tower level 0 or 3 .. base_level (little-endian values of
        2^(level - 3) bytes), constants in the base field.  base_level 3 is the call below."""
        return self.zerocheck_univariate_evals(n_vars, skip_rounds, columns, compositions, degrees, eq, max_domain_size, batch_coeff, base_level=base_level)

    def zerocheck_univariate_evals(self, n_vars, skip_rounds, columns, compositions, degrees, eq, max_domain_size, batch_coeff=None, base_level=None):
        """The univariate round of the univariate-skip zerocheck (bn_zerocheck_univariate_evals; prove/univariate.rs:235-507).
        columns: [(DevSlice of packed values, tower_level 0 or 3)] of 2^n_vars values each; compositions: step lists over B8;
        degrees: one per composition; eq: DevSlice of the 2^(n_vars - skip_rounds) expanded zerocheck challenges.  Returns per
        composition the list of P_c(omega_j), 2^skip_rounds <= j < max_domain_size -- or, with batch_coeff, the one list of
        sum_c batch_coeff^c P_c.  base_level (None: this entry point) selects bn_zerocheck_univariate_evals_base."""
        mls = (HalMultilinear * max(1, len(columns)))()
        for i, (sl, level) in enumerate(columns):
            mls[i].kind, mls[i].tower_level, mls[i].d_evals, mls[i].len, mls[i].n_vars_ml = HAL_ML_TRANSPARENT, level, sl.ptr, sl.len, n_vars
        flat, offs = [], [0]
        for steps in compositions:
            flat += list(steps)
            offs.append(len(flat))
        st = make_steps(flat)
        off_arr = (C.c_uint32 * len(offs))(*offs)
        deg_arr = (C.c_uint32 * max(1, len(degrees)))(*degrees)
        n_out = max(0, max_domain_size - (1 << skip_rounds))
        out = (F128 * max(1, n_out if batch_coeff is not None else n_out * len(compositions)))()
        bc = to_f128(batch_coeff) if batch_coeff is not None else None
        tail = (mls, len(columns), st, off_arr, deg_arr, len(compositions), eq.ptr if eq is not None else None, eq.len if eq is not None else 0,
                max_domain_size, C.byref(bc) if bc is not None else None, out)
        if base_level is None:
            _check(lib().bn_zerocheck_univariate_evals(self._h, n_vars, skip_rounds, *tail))
        else:
            _check(lib().bn_zerocheck_univariate_evals_base(self._h, base_level, n_vars, skip_rounds, *tail))
        if batch_coeff is not None:
            return [from_f128(out[i]) for i in range(n_out)]
        return [[from_f128(out[c * n_out + i]) for i in range(n_out)] for c in range(len(compositions))]

    def fri_fold(self, s_evals, tw_level, log_domain, log_len, log_batch_size, challenges, data_in, data_out):
        ch = _f128_array(list(challenges))
        _check(
            lib().bn_fri_fold(
                self._h, s_evals.ctypes.data_as(C.POINTER(C.c_uint64)), tw_level, log_domain, log_len, log_batch_size,
                ch, len(challenges), data_in.ptr, data_in.len, data_out.ptr, data_out.len,
            )
        )

    # ---- Merkle commitment with Groestl-256 (include/binius_amd.h; digests are 2 arena elements each)
    def merkle_build(self, elems, batch_size, nodes):
        """nodes: DevSlice of 2 * (2 * n_leaves - 1) elements receiving the flattened tree."""
        if batch_size and elems.len % batch_size == 0 and nodes.len != 2 * (2 * (elems.len // batch_size) - 1):
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: merkle_build: nodes must hold 2 * n_leaves - 1 digests")
        _check(lib().bn_merkle_build(self._h, elems.ptr, elems.len, batch_size, nodes.ptr))

    def groestl256_leaves(self, elems, batch_size, digests):
        if batch_size and elems.len % batch_size == 0 and digests.len != 2 * (elems.len // batch_size):
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: groestl256_leaves: digests must hold one digest per batch")
        _check(lib().bn_groestl256_leaves(self._h, elems.ptr, elems.len, batch_size, digests.ptr))

    def groestl256_compress_layer(self, prev, nxt):
        if prev.len != 2 * nxt.len:
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: compress_layer: the next layer is half the previous one")
        _check(lib().bn_groestl256_compress_layer(self._h, prev.ptr, nxt.len // 2, nxt.ptr))

    def gather_d2h(self, src, offsets, item_elems):
        """(len(offsets), item_elems, 2) uint64 array: src[offsets[i] : offsets[i] + item_elems] for every i."""
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(offs) and int(offs.max()) + item_elems > src.len:
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: gather: item out of range")
        out = np.zeros((len(offs), item_elems, 2), dtype=np.uint64)
        _check(lib().bn_gather_d2h(self._h, src.ptr, offs.ctypes.data_as(C.POINTER(C.c_uint64)), len(offs), item_elems, out.ctypes.data))
        return out

    def compute_composite(self, inputs, output, composition):
        rows = (C.c_void_p * max(1, len(inputs)))(*[r.ptr for r in inputs])
        row_len = inputs[0].len if inputs else 0
        for r in inputs:
            assert r.len == row_len  # SlicesBatch::new
        _check(lib().bn_compute_composite(self._h, rows, len(inputs), row_len, output.ptr, output.len, composition.handle))

    def compute_composite_tower(self, inputs, output, expr, n_values):
        """bn_compute_composite with an expression of expr_compile_tower: inputs[v] holds n_values values packed at the expression's
        input level v (at least one element), output n_values values at its output level."""
        rows = (C.c_void_p * max(1, len(inputs)))(*[r.ptr for r in inputs])
        _check(lib().bn_compute_composite(self._h, rows, len(inputs), n_values, output.ptr, n_values, expr.handle))

    def compute_composite_tower_batch(self, rows, arena, batch):
        """bn_compute_composite with a batch of expr_compile_tower_batch: rows are the input columns of all jobs (job j's input v is
        rows[first_row_j + v]), arena the slice the jobs' out_offsets count from.  One launch."""
        ptrs = (C.c_void_p * max(1, len(rows)))(*[r.ptr for r in rows])
        _check(lib().bn_compute_composite(self._h, ptrs, len(rows), arena.len, arena.ptr, arena.len, batch.handle))

    def pairwise_product_reduce(self, inp, round_outputs):
        outs = (C.c_void_p * max(1, len(round_outputs)))(*[r.ptr for r in round_outputs])
        lens = (C.c_uint64 * max(1, len(round_outputs)))(*[r.len for r in round_outputs])
        _check(lib().bn_pairwise_product_reduce(self._h, inp.ptr, inp.len, outs, lens, len(round_outputs)))

    def product_tree_layers(self, n_vars, inputs, arenas):
        """Every layer of a batch of halves-product trees (bn_product_tree_layers; gkr_gpa/gkr_gpa.rs:38-90).  n_vars: one per
        tree; inputs: DevSlices of up to 2^n_vars elements (None = empty; the absent tail counts as ONE); arenas: DevSlices of
        2^n_vars elements receiving layer j at [2^j, 2^(j+1)) (None allowed for n_vars = 0).  Returns the products."""
        n = len(n_vars)
        nv = (C.c_uint32 * max(1, n))(*n_vars)
        ins = (C.c_void_p * max(1, n))(*[(x.ptr if x is not None else None) for x in inputs])
        lens = (C.c_uint64 * max(1, n))(*[(x.len if x is not None else 0) for x in inputs])
        for t, a in enumerate(arenas):
            if a is not None and a.len != (1 << n_vars[t]) and n_vars[t] <= 28:
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: product tree: an arena holds 2^n_vars elements")
        outs = (C.c_void_p * max(1, n))(*[(a.ptr if a is not None else None) for a in arenas])
        prod = (F128 * max(1, n))()
        _check(lib().bn_product_tree_layers(self._h, n, nv, ins, lens, outs, prod))
        return [from_f128(prod[t]) for t in range(n)]

    def pad_with_ones(self, log_lens, srcs, dsts):
        """dsts[t] = srcs[t] followed by ONEs up to 2^log_lens[t] elements, every array in one launch (bn_pad_with_ones)."""
        n = len(log_lens)
        ll = (C.c_uint32 * max(1, n))(*log_lens)
        ins = (C.c_void_p * max(1, n))(*[(x.ptr if x is not None else None) for x in srcs])
        lens = (C.c_uint64 * max(1, n))(*[(x.len if x is not None else 0) for x in srcs])
        outs = (C.c_void_p * max(1, n))(*[d.ptr for d in dsts])
        _check(lib().bn_pad_with_ones(self._h, n, ll, ins, lens, outs))

    def exp_circuit_layers(self, n_vars, bit_columns, bases, arenas, kinds=None):
        """Every layer of a batch of exponentiation circuits in one launch (bn_exp_circuit_layers; gkr_exp/witness.rs:31-110, 139-156,
        258-284).  Per witness: n_vars; bit_columns: its DevSlices e_0 (least significant) .. e_{w-1}, each a packed B1 multilinear
        (bit i = bit i & 127 of element i >> 7; one element for n_vars < 7); bases: an int (the constant base g: static) or a
        DevSlice of 2^n_vars elements (dynamic); arenas: a DevSlice of w * 2^n_vars elements receiving layer k at k * 2^n_vars.
        kinds overrides the kind inferred from `bases` (0 static, 1 dynamic)."""
        n = len(n_vars)
        nv = (C.c_uint32 * max(1, n))(*n_vars)
        wd = (C.c_uint32 * max(1, n))(*[len(b) for b in bit_columns])
        if kinds is None:
            kinds = [0 if isinstance(b, int) else 1 for b in bases]
        kd = (C.c_uint32 * max(1, n))(*kinds)
        flat = [(c.ptr if c is not None else None) for cols in bit_columns for c in cols]
        cols = (C.c_void_p * max(1, len(flat)))(*flat)
        sb = (F128 * max(1, n))(*[to_f128(b if isinstance(b, int) else 0) for b in bases])
        db = (C.c_void_p * max(1, n))(*[(None if b is None or isinstance(b, int) else b.ptr) for b in bases])
        for t, a in enumerate(arenas):
            if a is not None and n_vars[t] <= 28 and a.len != len(bit_columns[t]) << n_vars[t]:
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: exp circuit: an arena holds width * 2^n_vars elements")
        outs = (C.c_void_p * max(1, n))(*[(a.ptr if a is not None else None) for a in arenas])
        _check(lib().bn_exp_circuit_layers(self._h, n, nv, wd, kd, cols, sb, db, outs))

    def bits_to_b128(self, log_lens, srcs, dsts):
        """dsts[t][i] = bit i of srcs[t] ? ONE : ZERO for i < 2^log_lens[t], every array in one launch (bn_bits_to_b128)."""
        n = len(log_lens)
        ll = (C.c_uint32 * max(1, n))(*log_lens)
        ins = (C.c_void_p * max(1, n))(*[(x.ptr if x is not None else None) for x in srcs])
        outs = (C.c_void_p * max(1, n))(*[(d.ptr if d is not None else None) for d in dsts])
        _check(lib().bn_bits_to_b128(self._h, n, ll, ins, outs))

    def exp_counters(self):
        """Accepted bn_exp_circuit_layers calls of this context, the kernel launches they made, and the launches of bn_bits_to_b128
        (bn_exp_counters).  Rejected calls count nowhere."""
        c = (C.c_uint64 * 3)()
        _check(lib().bn_exp_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "bits_launches": int(c[2])}

    def flush_witness_batch(self, n_vars, selectors, columns, const_terms, outs):
        """The masked witnesses of a batch of channel flushes in one launch (bn_flush_witness_batch; make_masked_flush_witnesses,
        constraint_system/prove.rs:671-881).  Per flush: n_vars; selectors: its DevSlices (packed B1 columns); columns: its
        (DevSlice, tower_level, coefficient) triples, the coefficient an int (the entry's mixing power); const_terms: an int;
        outs: a DevSlice of 2^n_vars elements, written below the returned prefix length only.  Returns the prefix lengths."""
        n = len(n_vars)
        nv = (C.c_uint32 * max(1, n))(*n_vars)
        ns = (C.c_uint32 * max(1, n))(*[len(s) for s in selectors])
        nc = (C.c_uint32 * max(1, n))(*[len(c) for c in columns])
        flat_s = [(s.ptr if s is not None else None) for sel in selectors for s in sel]
        flat_c = [c for cols in columns for c in cols]
        sp = (C.c_void_p * max(1, len(flat_s)))(*flat_s)
        cp = (C.c_void_p * max(1, len(flat_c)))(*[(c[0].ptr if c[0] is not None else None) for c in flat_c])
        lv = (C.c_uint32 * max(1, len(flat_c)))(*[c[1] for c in flat_c])
        cf = (F128 * max(1, len(flat_c)))(*[to_f128(c[2]) for c in flat_c])
        ct = (F128 * max(1, n))(*[to_f128(c) for c in const_terms])
        for t, o in enumerate(outs):
            if o is not None and n_vars[t] <= 28 and o.len != 1 << n_vars[t]:
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: flush witness: an output holds 2^n_vars elements")
        op = (C.c_void_p * max(1, n))(*[(o.ptr if o is not None else None) for o in outs])
        lens = (C.c_uint64 * max(1, n))()
        _check(lib().bn_flush_witness_batch(self._h, n, nv, ns, sp, nc, cp, lv, cf, ct, op, lens))
        return [int(lens[t]) for t in range(n)]

    def flush_counters(self):
        """bn_flush_counters: accepted bn_flush_witness_batch calls, the kernel launches they made, the flushes they served and how
        many of those ran in more than one pass of nibble tables.  Rejected calls count nowhere."""
        c = (C.c_uint64 * 4)()
        _check(lib().bn_flush_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "flushes": int(c[2]), "multipass": int(c[3])}

    def partial_eval_high_batch(self, columns, query, query_vars, outs):
        """A batch of columns evaluated at the high coordinates of one point (bn_partial_eval_high_batch; evaluate_partial_high of
        every inner column of an evalcheck round, evalcheck/subclaims.rs:356-439).  columns: (DevSlice, tower_level, n_vars) per
        column; query: the DevSlice of the 2^query_vars-element tensor expansion; outs[c]: a DevSlice of 2^(n_vars - query_vars)
        elements that receives what fold_left(column, level, query, out) would write."""
        n = len(columns)
        if len(outs) != n:
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: one output per column")
        cols = (PeColumn * max(1, n))(*[PeColumn(c[0].ptr if c[0] is not None else None, c[1], c[2]) for c in columns])
        for c, o in zip(columns, outs):
            if o is not None and query_vars <= c[2] <= 40 and o.len != 1 << (c[2] - query_vars):
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: output has the wrong number of elements")
        op = (C.c_void_p * max(1, n))(*[(o.ptr if o is not None else None) for o in outs])
        _check(lib().bn_partial_eval_high_batch(self._h, C.cast(cols, C.c_void_p), n, query.ptr if query is not None else None, query_vars, op))

    def partial_eval_counters(self):
        """bn_partial_eval_counters: accepted bn_partial_eval_high_batch calls, launches of the partial-evaluation kernels (routed
        bn_fold_left calls included), columns they served, columns that went to the fold_left kernels, the largest number of
        workgroups that shared one column in the last call, bn_fold_left calls routed to the kernel.  Rejected calls count nowhere."""
        c = (C.c_uint64 * 6)()
        _check(lib().bn_partial_eval_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "cols_kernel": int(c[2]), "cols_fallback": int(c[3]), "max_share": int(c[4]),
                "fold_left_routed": int(c[5])}

    def partial_eval_high_lincomb_batch(self, jobs, query, query_vars, outs):
        """The projection of partial_eval_high_batch for linear combinations of columns that are never materialised
        (bn_partial_eval_high_lincomb_batch; try_build_partial_eval, evalcheck/subclaims.rs:305-346).  jobs: (n_vars, terms, offset) per
        job, terms a list of (column DevSlice, tower_level, coeff), coefficients and offsets as ints; query: the DevSlice of the
        2^query_vars-element tensor expansion; outs[j]: a DevSlice of 2^(n_vars - query_vars) elements that receives
        offset + sum_t coeff_t * fold_left(column_t, level_t, query)."""
        n = len(jobs)
        if len(outs) != n:
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: one output per job")
        table, terms = [], []
        for n_vars, tms, offset in jobs:
            table.append(PelJob(n_vars, len(terms), len(tms), 0, to_f128(offset)))
            terms += [PelTerm(t[0].ptr if t[0] is not None else None, t[1], 0, to_f128(t[2])) for t in tms]
        for jb, o in zip(jobs, outs):
            if o is not None and query_vars <= jb[0] <= 40 and o.len != 1 << (jb[0] - query_vars):
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: output has the wrong number of elements")
        op = (C.c_void_p * max(1, n))(*[(o.ptr if o is not None else None) for o in outs])
        self.partial_eval_high_lincomb_raw((PelJob * max(1, n))(*table), n, (PelTerm * max(1, len(terms)))(*terms), len(terms), query, query_vars, op)

    def partial_eval_high_lincomb_raw(self, jobs, n_jobs, terms, n_terms, query, query_vars, outs):
        """bn_partial_eval_high_lincomb_batch on caller-built PelJob / PelTerm arrays (outs: a c_void_p array), nothing checked here."""
        _check(lib().bn_partial_eval_high_lincomb_batch(self._h, C.cast(jobs, C.c_void_p) if jobs is not None else None, n_jobs,
                                                        C.cast(terms, C.c_void_p) if terms is not None else None, n_terms,
                                                        query.ptr if query is not None else None, query_vars, outs))

    def partial_eval_lincomb_counters(self):
        """bn_partial_eval_lincomb_counters: accepted bn_partial_eval_high_lincomb_batch calls, the kernel launches they made, jobs, terms,
        classes (row loops planned), jobs served by the one-thread-per-output form, the largest number of workgroups that shared one job
        in the last call.  Rejected calls count nowhere."""
        c = (C.c_uint64 * 7)()
        _check(lib().bn_partial_eval_lincomb_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "jobs": int(c[2]), "terms": int(c[3]), "classes": int(c[4]), "jobs_fallback": int(c[5]),
                "max_share": int(c[6])}

    def univariate_fold_batch(self, columns, k, coeffs, outs):
        """The fold of the univariate round of the univariate-skip zerocheck for a batch of columns in one launch
        (bn_univariate_fold_batch; fold_univariate_round, sumcheck/prove/zerocheck.rs:384-434).  columns: (DevSlice, tower_level,
        n_vars) per column, level 0 or 3; k = skip_rounds; coeffs: the 2^k coefficients as ints (host); outs[c]: a DevSlice of
        2^(n_vars - k) elements that receives what fold_right(column, level, coeffs, out) would write."""
        n = len(columns)
        if len(outs) != n:
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: one output per column")
        coeffs = list(coeffs)
        if 0 <= k <= 8 and len(coeffs) != 1 << k:
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: univariate fold: 2^skip_rounds coefficients")
        cols = (PeColumn * max(1, n))(*[PeColumn(c[0].ptr if c[0] is not None else None, c[1], c[2]) for c in columns])
        for c, o in zip(columns, outs):
            if o is not None and 1 <= k <= c[2] <= 40 and o.len != 1 << (c[2] - k):
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: output has the wrong number of elements")
        op = (C.c_void_p * max(1, n))(*[(o.ptr if o is not None else None) for o in outs])
        _check(lib().bn_univariate_fold_batch(self._h, C.cast(cols, C.c_void_p), n, k, _f128_array(coeffs), op))

    def univariate_fold_counters(self):
        """bn_univariate_fold_counters: accepted bn_univariate_fold_batch calls, the kernel launches they made, the columns they
        served.  Rejected calls count nowhere."""
        c = (C.c_uint64 * 3)()
        _check(lib().bn_univariate_fold_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "columns": int(c[2])}

    def ring_switch_eq_ind_batch(self, jobs, coeffs, outs):
        """Every ring-switch equality indicator of a call in one launch (bn_ring_switch_eq_ind_batch; RingSwitchEqInd, ring_switch/
        eq_ind.rs:81-147).  jobs: (query DevSlice, n_vars, kappa, mixing_coeff) per job, the query the 2^n_vars-element tensor
        expansion of the job's suffix, the coefficient an int; coeffs: the row-batch coefficients as ints (host), a power of two of
        them and at least 2^kappa; outs[j]: a DevSlice of 2^n_vars elements that receives sum_i coeffs[i] * limb_i(mixing * query[x])."""
        n = len(jobs)
        if len(outs) != n:
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: one output per job")
        coeffs = list(coeffs)
        for jb, o in zip(jobs, outs):
            if 0 <= jb[1] <= 40 and ((jb[0] is not None and jb[0].len != 1 << jb[1]) or (o is not None and o.len != 1 << jb[1])):
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: ring switch: a query and an output hold 2^n_vars elements")
        table = (RsJob * max(1, n))(*[RsJob(jb[0].ptr if jb[0] is not None else None, jb[1], jb[2], to_f128(jb[3])) for jb in jobs])
        op = (C.c_void_p * max(1, n))(*[(o.ptr if o is not None else None) for o in outs])
        _check(lib().bn_ring_switch_eq_ind_batch(self._h, C.cast(table, C.c_void_p), n, _f128_array(coeffs), len(coeffs), op))

    def ring_switch_counters(self):
        """bn_ring_switch_counters: accepted bn_ring_switch_eq_ind_batch calls, the kernel launches they made, the jobs they served,
        the distinct query pointers among them.  Rejected calls count nowhere."""
        c = (C.c_uint64 * 4)()
        _check(lib().bn_ring_switch_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "jobs": int(c[2]), "queries": int(c[3])}

    def mle_evaluate_batch(self, jobs, points):
        """A batch of columns evaluated at their whole claim points in one call (bn_mle_evaluate_batch; the first step of
        EvalcheckProver::prove, evalcheck/prove.rs:191-275, 812-879).  points: (lo DevSlice, lo_vars, hi DevSlice, hi_vars) per point,
        the tensor expansions of its first lo_vars and its other hi_vars coordinates; jobs: (column DevSlice, tower_level, n_vars,
        point_index) per job.  Returns the evaluations as ints, in job order."""
        n, m = len(jobs), len(points)
        for pt in points:
            if (pt[0] is not None and 0 <= pt[1] <= 40 and pt[0].len != 1 << pt[1]) or (pt[2] is not None and 0 <= pt[3] <= 40 and pt[2].len != 1 << pt[3]):
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: mle evaluate: a table holds 2^vars elements")
        pts = (MePoint * max(1, m))(*[MePoint(pt[0].ptr if pt[0] is not None else None, pt[2].ptr if pt[2] is not None else None, pt[1], pt[3]) for pt in points])
        table = (MeJob * max(1, n))(*[MeJob(jb[0].ptr if jb[0] is not None else None, jb[1], jb[2], jb[3], 0) for jb in jobs])
        out = (F128 * max(1, n))()
        _check(lib().bn_mle_evaluate_batch(self._h, C.cast(table, C.c_void_p), n, C.cast(pts, C.c_void_p), m, out))
        return [from_f128(out[j]) for j in range(n)]

    def mle_evaluate_counters(self):
        """bn_mle_evaluate_counters: accepted bn_mle_evaluate_batch calls, the kernel launches they made, the jobs they served, the
        largest number of workgroups that shared one job in the last call.  Rejected calls count nowhere."""
        c = (C.c_uint64 * 4)()
        _check(lib().bn_mle_evaluate_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "jobs": int(c[2]), "max_share": int(c[3])}

    def merge_multilins(self, multilins, message, total_vars, log_repeats=0):
        """merge_multilins (piop/prove.rs:78-118) of multilinears on the device (bn_merge_multilins): multilins are DevSlices of
        2^n_vars elements, ascending by length; message, a DevSlice of 2^(total_vars + log_repeats) elements, receives 2^log_repeats
        copies of: the multilinears in reverse order, each with bit-reversed indices, then zeros up to 2^total_vars."""
        n = len(multilins)
        n_vars = []
        for m in multilins:
            if m is not None and (m.len == 0 or m.len & (m.len - 1)):
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: merge_multilins: a multilinear holds 2^n_vars elements")
            n_vars.append(m.len.bit_length() - 1 if m is not None else 0)
        if message is not None and 0 <= total_vars + log_repeats < 48 and message.len != 1 << (total_vars + log_repeats):
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: merge_multilins: the message holds 2^(total_vars + log_repeats) elements")
        nv = (C.c_uint32 * max(1, n))(*n_vars)
        ptrs = (C.c_void_p * max(1, n))(*[(m.ptr if m is not None else None) for m in multilins])
        _check(lib().bn_merge_multilins(self._h, n, nv, ptrs, message.ptr if message is not None else None, total_vars, log_repeats))

    def merge_counters(self):
        """bn_merge_counters: accepted bn_merge_multilins calls, the kernel launches they made, the jobs they served (multilinears and
        zero tails), the tiled and the small multilinears among them.  Rejected calls count nowhere."""
        c = (C.c_uint64 * 5)()
        _check(lib().bn_merge_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "jobs": int(c[2]), "jobs_tiled": int(c[3]), "jobs_small": int(c[4])}

    @staticmethod
    def derive_job_table(jobs):
        """The arguments of bn_derive_columns_batch, marshalled once: (DeriveJob array, n_jobs, c_void_p term array, n_terms) for
        derive_columns_raw.  jobs: dicts with kind ("shifted", "repeating", "zero_padded", "xor"), level, n_vars, out (a DevSlice of
        2^(n_vars + level - 7) elements) and, by kind: inner (DevSlice), block_size, shift_offset, variant ("circular_left", "logical_left",
        "logical_right"); inner, inner_n_vars; inner, inner_n_vars, start_index, nonzero_index; terms (DevSlices of the output's level and
        n_vars), offset (an int of the output's level)."""
        kinds = {"shifted": DERIVE_SHIFTED, "repeating": DERIVE_REPEATING, "zero_padded": DERIVE_ZERO_PADDED, "xor": DERIVE_XOR_COMBINATION}
        variants = {"circular_left": SHIFT_CIRCULAR_LEFT, "logical_left": SHIFT_LOGICAL_LEFT, "logical_right": SHIFT_LOGICAL_RIGHT}
        table, terms = [], []
        for jb in jobs:
            out, inner = jb.get("out"), jb.get("inner")
            if out is not None and jb["n_vars"] <= 40 and jb["level"] <= 7 and jb["n_vars"] + jb["level"] >= 7 and out.len != 1 << (jb["n_vars"] + jb["level"] - 7):
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: output has the wrong number of elements")
            tms = jb.get("terms", [])
            table.append(DeriveJob(kinds.get(jb["kind"], jb["kind"]), jb["level"], jb["n_vars"], jb.get("inner_n_vars", 0), inner.ptr if inner is not None else None,
                                   out.ptr if out is not None else None, jb.get("block_size", 0), variants.get(jb.get("variant", 0), jb.get("variant", 0)),
                                   jb.get("shift_offset", 0), jb.get("start_index", 0), jb.get("reserved", 0), jb.get("nonzero_index", 0), len(terms), len(tms),
                                   to_f128(jb.get("offset", 0))))
            terms += [(t.ptr if t is not None else None) for t in tms]
        return (DeriveJob * max(1, len(table)))(*table), len(table), (C.c_void_p * max(1, len(terms)))(*terms), len(terms)

    def derive_columns_batch(self, jobs):
        """The virtual columns of a constraint system built on the device in one launch (bn_derive_columns_batch; validate.rs:151-279,
        fold.rs:27-77).  jobs: as derive_job_table takes them."""
        self.derive_columns_raw(*self.derive_job_table(jobs))

    def derive_columns_raw(self, jobs, n_jobs, terms, n_terms):
        """bn_derive_columns_batch on a caller-built DeriveJob array and c_void_p term array, nothing checked here."""
        _check(lib().bn_derive_columns_batch(self._h, C.cast(jobs, C.c_void_p) if jobs is not None else None, n_jobs, terms, n_terms))

    def derive_counters(self):
        """bn_derive_counters: accepted bn_derive_columns_batch calls, the kernel launches they made, the jobs they served.  Rejected
        calls count nowhere."""
        c = (C.c_uint64 * 3)()
        _check(lib().bn_derive_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "jobs": int(c[2])}

    @staticmethod
    def generate_job_table(jobs):
        """The arguments of bn_generate_columns_batch, marshalled once: (GenerateJob array, n_jobs) for generate_columns_raw.  jobs: dicts
        with kind ("projected_bits", "constant", "step_down", "step_up", "select_row", "incrementing", "powers"), level, n_vars, out (a
        DevSlice of 2^(n_vars + level - 7) elements) and, by kind: inner (DevSlice), start_index, query_size, query_bits; value (an int of
        the level: a constant's value, a power's base); index."""
        table = []
        for jb in jobs:
            out, inner = jb.get("out"), jb.get("inner")
            if out is not None and jb["n_vars"] <= 40 and jb["level"] <= 7 and jb["n_vars"] + jb["level"] >= 7 and out.len != 1 << (jb["n_vars"] + jb["level"] - 7):
                raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: output has the wrong number of elements")
            table.append(GenerateJob(GEN_KINDS.get(jb["kind"], jb["kind"]), jb["level"], jb["n_vars"], jb.get("start_index", 0), inner.ptr if inner is not None else None,
                                     out.ptr if out is not None else None, jb.get("query_size", 0), jb.get("reserved", 0), jb.get("query_bits", 0), jb.get("index", 0),
                                     to_f128(jb.get("value", 0))))
        return (GenerateJob * max(1, len(table)))(*table), len(table)

    def generate_columns_batch(self, jobs):
        """The projected-bit, transparent and incrementing columns of a constraint system written on the device in one launch
        (bn_generate_columns_batch).  jobs: as generate_job_table takes them."""
        self.generate_columns_raw(*self.generate_job_table(jobs))

    def generate_columns_raw(self, jobs, n_jobs):
        """bn_generate_columns_batch on a caller-built GenerateJob array, nothing checked here."""
        _check(lib().bn_generate_columns_batch(self._h, C.cast(jobs, C.c_void_p) if jobs is not None else None, n_jobs))

    def generate_counters(self):
        """bn_generate_counters: accepted bn_generate_columns_batch calls, the kernel launches they made, the jobs they served.  Rejected
        calls count nowhere."""
        c = (C.c_uint64 * 3)()
        _check(lib().bn_generate_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "jobs": int(c[2])}

    def fri_query_openings(self, oracles, terminate, indices, index_bits, out_elems=None):
        """bn_fri_query_openings: the decommitment of FRIFolder::finish_proof (fri/prove.rs:483-507) in one launch.  oracles: tuples
        (codeword DevSlice, node-array DevSlice, log_n_cosets, log_coset_size, layer_depth, index_shift); terminate: the DevSlice of the
        terminate codeword; indices: the query indices, each below 2^index_bits.  Returns the (total, 2) uint64 block: terminate codeword,
        one layer per oracle, then per query and oracle the coset and its branch.  out_elems: what the caller believes the total is
        (default: bn_fri_query_proof_elems)."""
        table = fri_oracle_table(oracles)
        idx = np.ascontiguousarray(np.asarray(list(indices), dtype=np.uint64))
        t_len = terminate.len if terminate is not None else 0
        if out_elems is None:
            out_elems = fri_query_proof_elems(oracles, t_len, len(idx))[2]
        out = np.zeros((max(1, out_elems), 2), dtype=np.uint64)
        _check(lib().bn_fri_query_openings(self._h, C.cast(table, C.c_void_p), len(oracles), terminate.ptr if terminate is not None else None, t_len,
                                           idx.ctypes.data_as(C.POINTER(C.c_uint64)), len(idx), index_bits, out.ctypes.data, out_elems))
        return out[:out_elems]

    def fri_query_counters(self):
        """bn_fri_query_counters: accepted bn_fri_query_openings calls, the kernel launches they made, the (query, oracle) openings they
        served.  Rejected calls count nowhere."""
        c = (C.c_uint64 * 3)()
        _check(lib().bn_fri_query_counters(self._h, c))
        return {"calls": int(c[0]), "launches": int(c[1]), "openings": int(c[2])}

    # ---- accumulate_kernels / map_kernels
    def pick_log_chunks(self, mem_maps):
        mm = _make_maps(mem_maps)
        lc = C.c_uint32()
        _check(lib().bn_pick_log_chunks(mm, len(mem_maps), C.byref(lc)))
        return lc.value

    def record(self, map_fn, mem_maps):
        """Run the kernel-spec closure once against the recording executor."""
        log_chunks = self.pick_log_chunks(mem_maps)
        buffers = []
        for i, m in enumerate(mem_maps):
            if m[0] == "local":
                buffers.append(KernelBuffer(i, 0, (1 << m[1]) >> log_chunks, True))
            else:
                buffers.append(KernelBuffer(i, 0, m[1].len >> log_chunks, m[0] == "chunked_mut"))
        ke = KernelExec()
        rets = map_fn(ke, log_chunks, buffers)
        return ke.ops, [v.id for v in (rets or [])], log_chunks

    def kernel_launch(self, mem_maps, ops, ret_ids, log_chunks, d_out=None, want_host=True):
        mm = _make_maps(mem_maps)
        kops = (KOp * max(1, len(ops)))()
        keep = []
        for i, o in enumerate(ops):
            if o["op"] == "decl":
                kops[i].kind = KOP_DECL_VALUE
                kops[i].value = o["value"]
                kops[i].scalar = to_f128(o["init"])
            elif o["op"] == "sum":
                kops[i].kind = KOP_SUM_COMPOSITION
                kops[i].value = o["value"]
                kops[i].scalar = to_f128(o["coeff"])
                kops[i].expr = o["expr"].handle
                rows = (KSlice * max(1, len(o["rows"])))(*[KSlice(*r) for r in o["rows"]])
                keep.append(rows)
                kops[i].rows = rows
                kops[i].n_rows = len(o["rows"])
            elif o["op"] == "add":
                kops[i].kind = KOP_ADD
                kops[i].src1, kops[i].src2, kops[i].dst = KSlice(*o["src1"]), KSlice(*o["src2"]), KSlice(*o["dst"])
            else:
                kops[i].kind = KOP_ADD_ASSIGN
                kops[i].src1, kops[i].dst = KSlice(*o["src"]), KSlice(*o["dst"])
        rv = (C.c_uint32 * max(1, len(ret_ids)))(*ret_ids)
        h_out = (F128 * max(1, len(ret_ids)))()
        _check(
            lib().bn_kernel_launch(
                self._h, mm, len(mem_maps), kops, len(ops), rv, len(ret_ids), log_chunks,
                h_out if (want_host and ret_ids) else None, d_out,
            )
        )
        return [from_f128(h_out[i]) for i in range(len(ret_ids))] if want_host else None

    def accumulate_kernels(self, map_fn, mem_maps):
        ops, ret_ids, log_chunks = self.record(map_fn, mem_maps)
        return self.kernel_launch(mem_maps, ops, ret_ids, log_chunks)

    def map_kernels(self, map_fn, mem_maps):
        ops, _rets, log_chunks = self.record(map_fn, mem_maps)
        self.kernel_launch(mem_maps, ops, [], log_chunks)

    # ---- AdditiveNTT
    def ntt_forward(self, data_ptr, elem_level, tw_level, s_evals, log_domain, log_x, log_y, log_z, coset=0, coset_bits=0, skip_rounds=0):
        _check(
            lib().bn_ntt_forward(
                self._h, data_ptr, elem_level, tw_level, s_evals.ctypes.data_as(C.POINTER(C.c_uint64)), log_domain,
                log_x, log_y, log_z, coset, coset_bits, skip_rounds,
            )
        )

    def ntt_inverse(self, data_ptr, elem_level, tw_level, s_evals, log_domain, log_x, log_y, log_z, coset=0, coset_bits=0, skip_rounds=0):
        _check(
            lib().bn_ntt_inverse(
                self._h, data_ptr, elem_level, tw_level, s_evals.ctypes.data_as(C.POINTER(C.c_uint64)), log_domain,
                log_x, log_y, log_z, coset, coset_bits, skip_rounds,
            )
        )

    # raw byte copies for non-F128 NTT data
    def copy_bytes_h2d(self, src_np, dst_ptr):
        n16 = (src_np.nbytes + 15) // 16
        buf = np.zeros(n16 * 2, dtype=np.uint64)
        buf.view(np.uint8)[: src_np.nbytes] = src_np.view(np.uint8).reshape(-1)
        _check(lib().bn_copy_h2d(self._h, buf.ctypes.data, n16, dst_ptr, n16))

    def copy_bytes_d2h(self, src_ptr, dst_np):
        n16 = (dst_np.nbytes + 15) // 16
        buf = np.zeros(n16 * 2, dtype=np.uint64)
        _check(lib().bn_copy_d2h(self._h, src_ptr, n16, buf.ctypes.data, n16))
        dst_np.view(np.uint8).reshape(-1)[:] = buf.view(np.uint8)[: dst_np.nbytes]
        return dst_np
