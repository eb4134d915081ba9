//! Raw bindings of `include/binius_amd.h` -- one declaration per C entry point, same names, same
//! argument order, same widths (`tests/test_rust_shim_ffi.py` in the backend repository parses this block
//! and the header and compares them).
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

/// `bn_f128`: one little-endian u128 = `BinaryField128b` (crates/field/src/binary_field.rs:747).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct bn_f128 {
	pub lo: u64,
	pub hi: u64,
}

pub const BN_OK: c_int = 0;
pub const BN_ERR_INPUT_VALIDATION: c_int = 1;
pub const BN_ERR_ALLOC: c_int = 2;
pub const BN_ERR_DEVICE: c_int = 3;
pub const BN_ERR_CORE_LIB: c_int = 4;
/// a caller's transcript callback returned non-zero (`bnh_transcript`, include/binius_amd_host.h)
pub const BN_ERR_CALLBACK: c_int = 5;

/// Opaque context (stream, scratch, optional arena).
#[repr(C)]
pub struct bn_ctx {
	_private: [u8; 0],
}
/// Opaque compiled arithmetic circuit.
#[repr(C)]
pub struct bn_expr {
	_private: [u8; 0],
}

pub const BN_STEP_ADD: u32 = 0;
pub const BN_STEP_MUL: u32 = 1;
pub const BN_STEP_POW: u32 = 2;
pub const BN_STEP_CONST: u32 = 3;
pub const BN_STEP_VAR: u32 = 4;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bn_step {
	pub kind: u32,
	pub a: u32,
	pub b: u64,
	pub cst: bn_f128,
}

pub const BN_NTT_MAX_DIM: usize = 64;

pub const BN_MAP_CHUNKED: u32 = 0;
pub const BN_MAP_CHUNKED_MUT: u32 = 1;
pub const BN_MAP_LOCAL: u32 = 2;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_memmap {
	pub kind: u32,
	pub log_min_chunk_size: u32,
	pub d_data: *mut c_void,
	pub len: u64,
	pub log_size: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bn_kslice {
	pub buf: u32,
	pub off: u64,
	pub len: u64,
}

pub const BN_KOP_DECL_VALUE: u32 = 0;
pub const BN_KOP_SUM_COMPOSITION: u32 = 1;
pub const BN_KOP_ADD: u32 = 2;
pub const BN_KOP_ADD_ASSIGN: u32 = 3;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_kop {
	pub kind: u32,
	pub value: u32,
	pub scalar: bn_f128,
	pub expr: *const bn_expr,
	pub n_rows: u32,
	pub rows: *const bn_kslice,
	pub src1: bn_kslice,
	pub src2: bn_kslice,
	pub dst: bn_kslice,
}

pub const BN_PROF_N: usize = 11;
pub const BN_ARM_N: usize = 15;
pub const BN_FP4_N: usize = 7;
pub const BN_NTT_N: usize = 3;
pub const BN_FRI_N: usize = 6;
pub const BN_FOLD_N: usize = 16;
pub const BN_IP_N: usize = 4;
pub const BN_HALCNT_N: usize = 17;
pub const BN_EXP_N: usize = 3;
pub const BN_PE_N: usize = 6;
pub const BN_PE_CALLS: usize = 0;
pub const BN_PE_LAUNCHES: usize = 1;
pub const BN_PE_COLS_KERNEL: usize = 2;
pub const BN_PE_COLS_FALLBACK: usize = 3;
pub const BN_PE_MAX_SHARE: usize = 4;
pub const BN_PE_FOLD_LEFT_ROUTED: usize = 5;
pub const BN_PE_MAX_VARS: u32 = 40;
pub const BN_PEL_N: usize = 7;
pub const BN_PEL_CALLS: usize = 0;
pub const BN_PEL_LAUNCHES: usize = 1;
pub const BN_PEL_JOBS: usize = 2;
pub const BN_PEL_TERMS: usize = 3;
pub const BN_PEL_CLASSES: usize = 4;
pub const BN_PEL_JOBS_FALLBACK: usize = 5;
pub const BN_PEL_MAX_SHARE: usize = 6;
pub const BN_PEL_MAX_TERMS: u32 = 64;
pub const BN_UF_N: usize = 3;
pub const BN_UF_CALLS: usize = 0;
pub const BN_UF_LAUNCHES: usize = 1;
pub const BN_UF_COLS: usize = 2;
pub const BN_RS_N: usize = 4;
pub const BN_RS_CALLS: usize = 0;
pub const BN_RS_LAUNCHES: usize = 1;
pub const BN_RS_JOBS: usize = 2;
pub const BN_RS_QUERIES: usize = 3;
pub const BN_ME_N: usize = 4;
pub const BN_ME_CALLS: usize = 0;
pub const BN_ME_LAUNCHES: usize = 1;
pub const BN_ME_JOBS: usize = 2;
pub const BN_ME_MAX_SHARE: usize = 3;
pub const BN_ME_MAX_LO_VARS: u32 = 10;
pub const BN_ME_MAX_JOBS: u32 = 4096;
pub const BN_MERGE_N: usize = 5;
pub const BN_MERGE_CALLS: usize = 0;
pub const BN_MERGE_LAUNCHES: usize = 1;
pub const BN_MERGE_JOBS: usize = 2;
pub const BN_MERGE_JOBS_TILED: usize = 3;
pub const BN_MERGE_JOBS_SMALL: usize = 4;
pub const BN_MERGE_TILE_LOG2: u32 = 6;
pub const BN_FQ_N: usize = 3;
pub const BN_FQ_CALLS: usize = 0;
pub const BN_FQ_LAUNCHES: usize = 1;
pub const BN_FQ_OPENINGS: usize = 2;
pub const BN_FRI_QUERY_MAX_ORACLES: u32 = 32;
pub const BN_UNIVARIATE_FOLD_MAX_SKIP: u32 = 8;
pub const BN_EXP_STATIC: u32 = 0;
pub const BN_EXP_DYNAMIC: u32 = 1;
pub const BN_EXP_MAX_VARS: u32 = 28;
pub const BN_EXP_MAX_WIDTH: u32 = 128;

// ---- the old HAL (binius_hal::ComputationBackend) on device-resident multilinears
pub const BN_ORDER_LOW_TO_HIGH: u32 = 0;
pub const BN_ORDER_HIGH_TO_LOW: u32 = 1;
pub const BN_HAL_ML_FOLDED: u32 = 0;
pub const BN_HAL_ML_TRANSPARENT: u32 = 1;

/// One committed oracle of bn_fri_query_openings: the codeword, the flattened Merkle tree over its cosets, and where a query lands in it.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_fri_oracle {
	pub d_codeword: *const c_void,
	pub d_nodes: *const c_void,
	pub log_n_cosets: u32,
	pub log_coset_size: u32,
	pub layer_depth: u32,
	pub index_shift: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_pe_column {
	pub d_evals: *const c_void,
	pub tower_level: u32,
	pub n_vars: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_pel_term {
	pub d_evals: *const c_void,
	pub tower_level: u32,
	pub reserved: u32,
	pub coeff: bn_f128,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_pel_job {
	pub n_vars: u32,
	pub first_term: u32,
	pub n_terms: u32,
	pub reserved: u32,
	pub offset: bn_f128,
}

/// One virtual column of bn_derive_columns_batch (Shifted, Repeating, ZeroPadded, or a LinearCombination with unit coefficients).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_derive_job {
	pub kind: u32,
	pub tower_level: u32,
	pub n_vars: u32,
	pub inner_n_vars: u32,
	pub d_inner: *const c_void,
	pub d_out: *mut c_void,
	pub block_size: u32,
	pub shift_variant: u32,
	pub shift_offset: u64,
	pub start_index: u32,
	pub reserved: u32,
	pub nonzero_index: u64,
	pub first_term: u32,
	pub n_terms: u32,
	pub offset: bn_f128,
}
pub const BN_DERIVE_SHIFTED: u32 = 0;
pub const BN_DERIVE_REPEATING: u32 = 1;
pub const BN_DERIVE_ZERO_PADDED: u32 = 2;
pub const BN_DERIVE_XOR_COMBINATION: u32 = 3;
pub const BN_SHIFT_CIRCULAR_LEFT: u32 = 0;
pub const BN_SHIFT_LOGICAL_LEFT: u32 = 1;
pub const BN_SHIFT_LOGICAL_RIGHT: u32 = 2;
pub const BN_DERIVE_N: usize = 3;

/// bn_expr_compile_tower: the caps of a tower-typed expression; bn_compute_composite_counters: what its calls did.
pub const BN_TOWER_EXPR_MAX_STEPS: usize = 1024;
pub const BN_TOWER_EXPR_MAX_INPUTS: usize = 256;
pub const BN_TOWER_EXPR_MAX_LIVE: usize = 16;
pub const BN_CC_TOWER_CALLS: usize = 0;
pub const BN_CC_TOWER_LAUNCHES: usize = 1;
pub const BN_CC_TOWER_BITWISE: usize = 2;
pub const BN_CC_TOWER_VALUES: usize = 3;
pub const BN_CC_N: usize = 4;

/// bn_expr_compile_tower_batch: one job of a batch of tower-typed expressions (it crosses the C interface as BN_COMPOSE_JOB_DESC_WORDS
/// integers of `job_desc` and one of `out_offsets`); bn_compute_composite_batch_counters: what its calls did.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct bn_compose_job {
	pub expr: u32,
	pub first_row: u32,
	pub n_vars: u32,
	pub reserved: u32,
	pub out_offset: u64,
}
pub const BN_COMPOSE_BATCH_MAX_JOBS: usize = 4096;
pub const BN_COMPOSE_JOB_DESC_WORDS: usize = 4;
pub const BN_CCB_CALLS: usize = 0;
pub const BN_CCB_LAUNCHES: usize = 1;
pub const BN_CCB_JOBS: usize = 2;
pub const BN_CCB_PROGRAMS: usize = 3;
pub const BN_CCB_N: usize = 4;

/// One generated column of bn_generate_columns_batch (a projection at a hypercube vertex, a transparent that its parameters determine, or
/// the incrementing column).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_generate_job {
	pub kind: u32,
	pub tower_level: u32,
	pub n_vars: u32,
	pub start_index: u32,
	pub d_inner: *const c_void,
	pub d_out: *mut c_void,
	pub query_size: u32,
	pub reserved: u32,
	pub query_bits: u64,
	pub index: u64,
	pub value: bn_f128,
}
pub const BN_GEN_PROJECTED_BITS: u32 = 0;
pub const BN_GEN_CONSTANT: u32 = 1;
pub const BN_GEN_STEP_DOWN: u32 = 2;
pub const BN_GEN_STEP_UP: u32 = 3;
pub const BN_GEN_SELECT_ROW: u32 = 4;
pub const BN_GEN_INCREMENTING: u32 = 5;
pub const BN_GEN_POWERS: u32 = 6;
pub const BN_GENERATE_N: usize = 3;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_rs_job {
	pub d_query: *const c_void,
	pub n_vars: u32,
	pub kappa: u32,
	pub mixing_coeff: bn_f128,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_me_point {
	pub d_lo: *const c_void,
	pub d_hi: *const c_void,
	pub lo_vars: u32,
	pub hi_vars: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_me_job {
	pub d_evals: *const c_void,
	pub tower_level: u32,
	pub n_vars: u32,
	pub point: u32,
	pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_hal_multilinear {
	pub kind: u32,
	pub tower_level: u32,
	pub d_evals: *const c_void,
	pub len: u64,
	pub suffix_eval: bn_f128,
	pub n_vars_ml: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bn_hal_evaluator {
	pub composition: *const bn_expr,
	pub composition_at_infinity: *const bn_expr,
	pub eval_point_start: u32,
	pub eval_point_end: u32,
	pub d_eq_ind: *const c_void,
}

unsafe extern "C" {
	pub fn bn_last_error() -> *const c_char;
	pub fn bn_version() -> *const c_char;

	pub fn bn_ctx_create(device: c_int, arena_elems: u64, out: *mut *mut bn_ctx) -> c_int;
	pub fn bn_ctx_destroy(ctx: *mut bn_ctx) -> c_int;
	pub fn bn_arena_base(ctx: *mut bn_ctx, d_base: *mut *mut c_void, elems: *mut u64) -> c_int;
	pub fn bn_ctx_set_stream(ctx: *mut bn_ctx, hip_stream: *mut c_void) -> c_int;
	pub fn bn_sync(ctx: *mut bn_ctx) -> c_int;
	pub fn bn_ctx_get_stream(ctx: *mut bn_ctx, hip_stream: *mut *mut c_void) -> c_int;

	pub fn bn_copy_h2d(ctx: *mut bn_ctx, h_src: *const bn_f128, src_len: u64, d_dst: *mut c_void, dst_len: u64) -> c_int;
	pub fn bn_copy_d2h(ctx: *mut bn_ctx, d_src: *const c_void, src_len: u64, h_dst: *mut bn_f128, dst_len: u64) -> c_int;
	pub fn bn_copy_d2d(ctx: *mut bn_ctx, d_src: *const c_void, src_len: u64, d_dst: *mut c_void, dst_len: u64) -> c_int;
	pub fn bn_fill(ctx: *mut bn_ctx, d_dst: *mut c_void, n: u64, value: *const bn_f128) -> c_int;

	pub fn bn_expr_compile(ctx: *mut bn_ctx, steps: *const bn_step, n_steps: u64, out: *mut *mut bn_expr) -> c_int;
	pub fn bn_expr_free(expr: *mut bn_expr) -> c_int;
	pub fn bn_expr_n_vars(expr: *const bn_expr, n_vars: *mut u32) -> c_int;
	pub fn bn_expr_compile_tower(
		ctx: *mut bn_ctx,
		steps: *const bn_step,
		n_steps: u64,
		input_levels: *const u32,
		n_inputs: u32,
		out_level: u32,
		out: *mut *mut bn_expr,
	) -> c_int;
	pub fn bn_compute_composite_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_expr_compile_tower_batch(
		ctx: *mut bn_ctx,
		exprs: *const *const bn_expr,
		n_exprs: u32,
		job_desc: *const u32,
		out_offsets: *const u64,
		n_jobs: u32,
		out: *mut *mut bn_expr,
	) -> c_int;
	pub fn bn_compute_composite_batch_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;

	pub fn bn_extrapolate_line(ctx: *mut bn_ctx, d_evals_0: *mut c_void, n0: u64, d_evals_1: *const c_void, n1: u64, z: *const bn_f128) -> c_int;
	pub fn bn_extrapolate_line_batch(
		ctx: *mut bn_ctx,
		d_evals_0: *const *mut c_void,
		d_evals_1: *const *const c_void,
		count: u32,
		n: u64,
		z: *const bn_f128,
	) -> c_int;
	pub fn bn_extrapolate_line_batch_scaled(
		ctx: *mut bn_ctx,
		d_evals_0: *const *mut c_void,
		d_evals_1: *const *const c_void,
		count: u32,
		n: u64,
		z: *const bn_f128,
		scale_mask: u32,
		hi_scale: *const bn_f128,
	) -> c_int;
	pub fn bn_tensor_expand(ctx: *mut bn_ctx, d_data: *mut c_void, data_len: u64, log_n: u32, h_coords: *const bn_f128, k: u32) -> c_int;
	pub fn bn_inner_product(
		ctx: *mut bn_ctx,
		d_a: *const c_void,
		a_len: u64,
		tower_level: u32,
		d_b: *const c_void,
		b_len: u64,
		h_out: *mut bn_f128,
	) -> c_int;
	pub fn bn_fold_left(
		ctx: *mut bn_ctx,
		d_mat: *const c_void,
		mat_len: u64,
		tower_level: u32,
		d_vec: *const c_void,
		vec_len: u64,
		d_out: *mut c_void,
		out_len: u64,
	) -> c_int;
	pub fn bn_fold_right(
		ctx: *mut bn_ctx,
		d_mat: *const c_void,
		mat_len: u64,
		tower_level: u32,
		d_vec: *const c_void,
		vec_len: u64,
		d_out: *mut c_void,
		out_len: u64,
	) -> c_int;
	pub fn bn_fri_fold(
		ctx: *mut bn_ctx,
		h_s_evals: *const u64,
		tw_level: u32,
		log_domain: u32,
		log_len: u32,
		log_batch_size: u32,
		h_challenges: *const bn_f128,
		n_challenges: u32,
		d_in: *const c_void,
		in_len: u64,
		d_out: *mut c_void,
		out_len: u64,
	) -> c_int;
	pub fn bn_compute_composite(
		ctx: *mut bn_ctx,
		d_rows: *const *const c_void,
		n_rows: u32,
		row_len: u64,
		d_out: *mut c_void,
		out_len: u64,
		expr: *const bn_expr,
	) -> c_int;
	pub fn bn_pairwise_product_reduce(
		ctx: *mut bn_ctx,
		d_in: *const c_void,
		n: u64,
		d_round_outs: *const *mut c_void,
		round_lens: *const u64,
		n_rounds: u32,
	) -> c_int;
	pub fn bn_product_tree_layers(
		ctx: *mut bn_ctx,
		n_trees: u32,
		n_vars: *const u32,
		d_inputs: *const *const c_void,
		input_lens: *const u64,
		d_layers: *const *mut c_void,
		products_out: *mut bn_f128,
	) -> c_int;
	pub fn bn_pad_with_ones(
		ctx: *mut bn_ctx,
		n: u32,
		log_lens: *const u32,
		d_srcs: *const *const c_void,
		src_lens: *const u64,
		d_dsts: *const *mut c_void,
	) -> c_int;
	pub fn bn_exp_circuit_layers(
		ctx: *mut bn_ctx,
		n_witnesses: u32,
		n_vars: *const u32,
		widths: *const u32,
		kinds: *const u32,
		d_exponent_bits: *const *const c_void,
		static_bases: *const bn_f128,
		d_bases: *const *const c_void,
		d_layers: *const *mut c_void,
	) -> c_int;
	pub fn bn_bits_to_b128(ctx: *mut bn_ctx, n: u32, log_lens: *const u32, d_srcs: *const *const c_void, d_dsts: *const *mut c_void) -> c_int;
	pub fn bn_exp_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_flush_witness_batch(
		ctx: *mut bn_ctx,
		n_flushes: u32,
		n_vars: *const u32,
		n_selectors: *const u32,
		d_selectors: *const *const c_void,
		n_columns: *const u32,
		d_columns: *const *const c_void,
		tower_levels: *const u32,
		coeffs: *const bn_f128,
		const_terms: *const bn_f128,
		d_outs: *const *mut c_void,
		prefix_lens_out: *mut u64,
	) -> c_int;
	pub fn bn_flush_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_partial_eval_high_batch(
		ctx: *mut bn_ctx,
		cols: *const c_void,
		n_cols: u32,
		d_tensor_query: *const c_void,
		query_vars: u32,
		d_outs: *const *mut c_void,
	) -> c_int;
	pub fn bn_partial_eval_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_partial_eval_high_lincomb_batch(
		ctx: *mut bn_ctx,
		jobs: *const c_void,
		n_jobs: u32,
		terms: *const c_void,
		n_terms_total: u32,
		d_tensor_query: *const c_void,
		query_vars: u32,
		d_outs: *const *mut c_void,
	) -> c_int;
	pub fn bn_partial_eval_lincomb_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_univariate_fold_batch(
		ctx: *mut bn_ctx,
		cols: *const c_void,
		n_cols: u32,
		skip_rounds: u32,
		h_coeffs: *const bn_f128,
		d_outs: *const *mut c_void,
	) -> c_int;
	pub fn bn_univariate_fold_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_ring_switch_eq_ind_batch(
		ctx: *mut bn_ctx,
		jobs: *const c_void,
		n_jobs: u32,
		h_row_batch_coeffs: *const bn_f128,
		n_coeffs: u32,
		d_outs: *const *mut c_void,
	) -> c_int;
	pub fn bn_ring_switch_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_mle_evaluate_batch(
		ctx: *mut bn_ctx,
		jobs: *const c_void,
		n_jobs: u32,
		points: *const c_void,
		n_points: u32,
		h_out: *mut bn_f128,
	) -> c_int;
	pub fn bn_mle_evaluate_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_merge_multilins(
		ctx: *mut bn_ctx,
		n: u32,
		n_vars: *const u32,
		d_multilins: *const *const c_void,
		d_message: *mut c_void,
		total_vars: u32,
		log_repeats: u32,
	) -> c_int;
	pub fn bn_merge_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_derive_columns_batch(
		ctx: *mut bn_ctx,
		jobs: *const c_void,
		n_jobs: u32,
		d_terms: *const *const c_void,
		n_terms_total: u32,
	) -> c_int;
	pub fn bn_derive_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_generate_columns_batch(ctx: *mut bn_ctx, jobs: *const c_void, n_jobs: u32) -> c_int;
	pub fn bn_generate_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_fri_query_proof_elems(
		oracles: *const c_void,
		n_oracles: u32,
		terminate_elems: u64,
		n_queries: u64,
		header_elems_out: *mut u64,
		record_elems_out: *mut u64,
		total_elems_out: *mut u64,
	) -> c_int;
	pub fn bn_fri_query_openings(
		ctx: *mut bn_ctx,
		oracles: *const c_void,
		n_oracles: u32,
		d_terminate: *const c_void,
		terminate_elems: u64,
		indices: *const u64,
		n_queries: u64,
		index_bits: u32,
		h_out: *mut bn_f128,
		out_elems: u64,
	) -> c_int;
	pub fn bn_fri_query_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;

	pub fn bn_log_chunks_range(maps: *const bn_memmap, n_maps: u32, start: *mut u32, end: *mut u32) -> c_int;
	pub fn bn_pick_log_chunks(maps: *const bn_memmap, n_maps: u32, log_chunks: *mut u32) -> c_int;
	pub fn bn_kernel_launch(
		ctx: *mut bn_ctx,
		maps: *const bn_memmap,
		n_maps: u32,
		ops: *const bn_kop,
		n_ops: u32,
		ret_values: *const u32,
		n_ret: u32,
		log_chunks: u32,
		h_out: *mut bn_f128,
		d_out: *mut c_void,
	) -> c_int;

	pub fn bn_hal_round_evals(
		ctx: *mut bn_ctx,
		order: u32,
		n_vars: u32,
		d_tensor_query: *const c_void,
		query_vars: u32,
		mls: *const bn_hal_multilinear,
		n_mls: u32,
		evaluators: *const bn_hal_evaluator,
		n_evaluators: u32,
		h_nontrivial_points: *const bn_f128,
		n_points: u32,
		h_out: *mut bn_f128,
	) -> c_int;
	pub fn bn_hal_fold_multilinear(
		ctx: *mut bn_ctx,
		order: u32,
		n_vars: u32,
		ml: *const bn_hal_multilinear,
		challenge: *const bn_f128,
		d_tensor_query: *const c_void,
		query_vars: u32,
		d_out: *mut c_void,
		out_cap: u64,
		out_len: *mut u64,
	) -> c_int;
	pub fn bn_zerocheck_univariate_evals(
		ctx: *mut bn_ctx,
		n_vars: u32,
		skip_rounds: u32,
		mls: *const bn_hal_multilinear,
		n_mls: u32,
		steps: *const bn_step,
		step_offsets: *const u32,
		degrees: *const u32,
		n_comps: u32,
		d_eq: *const c_void,
		eq_len: u64,
		max_domain_size: u32,
		h_batch_coeff: *const bn_f128,
		h_out: *mut bn_f128,
	) -> c_int;
	pub fn bn_zerocheck_univariate_evals_base(
		ctx: *mut bn_ctx,
		base_level: u32,
		n_vars: u32,
		skip_rounds: u32,
		mls: *const bn_hal_multilinear,
		n_mls: u32,
		steps: *const bn_step,
		step_offsets: *const u32,
		degrees: *const u32,
		n_comps: u32,
		d_eq: *const c_void,
		eq_len: u64,
		max_domain_size: u32,
		h_batch_coeff: *const bn_f128,
		h_out: *mut bn_f128,
	) -> c_int;

	pub fn bn_ntt_forward(
		ctx: *mut bn_ctx,
		d_data: *mut c_void,
		elem_level: u32,
		tw_level: u32,
		h_s_evals: *const u64,
		log_domain: u32,
		log_x: u32,
		log_y: u32,
		log_z: u32,
		coset: u64,
		coset_bits: u32,
		skip_rounds: u32,
	) -> c_int;
	pub fn bn_ntt_inverse(
		ctx: *mut bn_ctx,
		d_data: *mut c_void,
		elem_level: u32,
		tw_level: u32,
		h_s_evals: *const u64,
		log_domain: u32,
		log_x: u32,
		log_y: u32,
		log_z: u32,
		coset: u64,
		coset_bits: u32,
		skip_rounds: u32,
	) -> c_int;
	pub fn bn_ntt_s_evals(tw_level: u32, log_domain: u32, h_s_evals: *mut u64) -> c_int;

	pub fn bn_scalar_mul(a: *const bn_f128, b: *const bn_f128, out: *mut bn_f128) -> c_int;
	pub fn bn_scalar_invert(a: *const bn_f128, out: *mut bn_f128) -> c_int;

	pub fn bn_groestl256_leaves(ctx: *mut bn_ctx, d_elems: *const c_void, n_elems: u64, batch_size: u64, d_digests: *mut c_void) -> c_int;
	pub fn bn_groestl256_compress_layer(ctx: *mut bn_ctx, d_prev: *const c_void, n_out: u64, d_next: *mut c_void) -> c_int;
	pub fn bn_merkle_build(ctx: *mut bn_ctx, d_elems: *const c_void, n_elems: u64, batch_size: u64, d_nodes: *mut c_void) -> c_int;
	pub fn bn_gather_d2h(ctx: *mut bn_ctx, d_src: *const c_void, h_offsets: *const u64, n_items: u64, item_elems: u64, h_out: *mut bn_f128) -> c_int;

	pub fn bn_timer_begin(ctx: *mut bn_ctx) -> c_int;
	pub fn bn_timer_end_ms(ctx: *mut bn_ctx, ms: *mut f32) -> c_int;
	pub fn bn_host_scratch(ctx: *mut bn_ctx, h_ptr: *mut *mut c_void, d_ptr: *mut *mut c_void, elems: *mut u64) -> c_int;
	pub fn bn_device_numa_node(device: c_int, node: *mut c_int) -> c_int;
	pub fn bn_xor_reduce(ctx: *mut bn_ctx, d_vals: *const c_void, n_groups: u32, group_len: u32, h_out: *mut bn_f128) -> c_int;
	pub fn bn_prof_begin(ctx: *mut bn_ctx) -> c_int;
	pub fn bn_prof_end(ctx: *mut bn_ctx, ms_by_class: *mut f64, launches_by_class: *mut u64) -> c_int;
	pub fn bn_arm_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_group_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_fp4_last_grids(ctx: *mut bn_ctx, grids: *mut u64) -> c_int;
	pub fn bn_ntt_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_fri_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_fold_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_inner_product_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	pub fn bn_hal_counters(ctx: *mut bn_ctx, counters: *mut u64) -> c_int;
	// cross-rank reduction of the round evaluations inside the kernels' finalize step (one process per GPU)
	pub fn bn_peer_create(ctx: *mut bn_ctx, world: u32, rank: u32, handle_out: *mut u8) -> c_int;
	pub fn bn_peer_connect(ctx: *mut bn_ctx, handles: *const u8) -> c_int;
	pub fn bn_peer_set_active(ctx: *mut bn_ctx, on: c_int) -> c_int;
	pub fn bn_peer_stats(ctx: *mut bn_ctx, stats: *mut u64) -> c_int;
	pub fn bn_host_tail_allow_peer(ctx: *mut bn_ctx, on: c_int) -> c_int;
	pub fn bn_host_tail_active(ctx: *mut bn_ctx, active: *mut c_int) -> c_int;
	pub fn bn_peer_destroy(ctx: *mut bn_ctx) -> c_int;
}

// ---- include/binius_amd_host.h, "Against a live transcript": the callback table, the `_live` form of every compiled prover that
// takes transcript samples, and the library's array-backed transcript.  `src/transcript.rs` adapts `ProverTranscript` to the table.
pub const BNH_TR_MESSAGE: u32 = 0;
pub const BNH_TR_DECOMMITMENT: u32 = 1;
pub const BNH_TR_EVENT_WRITE_MESSAGE: u32 = 0;
pub const BNH_TR_EVENT_WRITE_DECOMMITMENT: u32 = 1;
pub const BNH_TR_EVENT_SAMPLE: u32 = 2;
pub const BNH_TR_EVENT_SAMPLE_BITS: u32 = 3;

/// `bnh_transcript`: the caller's Fiat-Shamir transcript as three callbacks.  A callback returns 0, or non-zero to end the proof
/// with `BN_ERR_CALLBACK`; it runs on the calling thread and must not re-enter the library on the same context.
#[repr(C)]
pub struct bnh_transcript {
	pub user: *mut c_void,
	pub write: Option<unsafe extern "C" fn(user: *mut c_void, channel: u32, bytes: *const c_void, len: u64) -> c_int>,
	pub sample: Option<unsafe extern "C" fn(user: *mut c_void, out: *mut bn_f128, n: u32) -> c_int>,
	pub sample_bits: Option<unsafe extern "C" fn(user: *mut c_void, bits: u32, n: u32, out: *mut u64) -> c_int>,
}
/// Opaque array-backed transcript (`bnh_transcript_replay_*`).
#[repr(C)]
pub struct bnh_transcript_replay {
	_private: [u8; 0],
}

unsafe extern "C" {
	pub fn bnh_batch_sumcheck_prove_live(
		ctx: *mut bn_ctx, n_provers: u32, prover_desc: *const u32, d_multilins: *const *const c_void, comp_indices: *const u32, sums: *const bn_f128,
		d_scratch: *mut c_void, scratch_elems: u64, transcript: *const bnh_transcript, round_proofs_out: *mut bn_f128, final_evals_out: *mut bn_f128,
	) -> c_int;
	pub fn bnh_eqind_sumcheck_prove_live(
		ctx: *mut bn_ctx, n_vars: u32, n_mls: u32, d_multilins: *const *mut c_void, n_comps: u32, steps: *const bn_step, n_steps: *const u32,
		steps_inf: *const bn_step, n_steps_inf: *const u32, degrees: *const u32, sums: *const bn_f128, eq_ind_challenges: *const bn_f128, d_eq_ind: *mut c_void,
		eq_ind_elems: u64, transcript: *const bnh_transcript, round_coeffs_out: *mut bn_f128, final_evals_out: *mut bn_f128,
	) -> c_int;
	pub fn bnh_zerocheck_batch_prove_tower_live(
		ctx: *mut bn_ctx, n_tables: u32, skip_rounds: u32, n_vars: *const u32, n_cols: *const u32, d_cols: *const *const c_void, tower_levels: *const u32,
		n_comps: *const u32, steps: *const bn_step, n_steps: *const u32, steps_inf: *const bn_step, n_steps_inf: *const u32, degrees: *const u32,
		transcript: *const bnh_transcript, d_scratch: *mut c_void, scratch_elems: u64, message_out: *mut bn_f128, round_coeffs_out: *mut bn_f128,
		final_evals_out: *mut bn_f128, reduction_round_coeffs_out: *mut bn_f128, reduction_final_evals_out: *mut bn_f128, skipped_challenges_out: *mut bn_f128,
		unskipped_challenges_out: *mut bn_f128, concat_multilinear_evals_out: *mut bn_f128, phase_ms_out: *mut f64, phase_calls_out: *mut u64,
	) -> c_int;
	pub fn bnh_gkr_gpa_prove_live(
		ctx: *mut bn_ctx, n_claims: u32, n_vars: *const u32, d_inputs: *const *const c_void, input_lens: *const u64, d_arenas: *const *mut c_void,
		d_scratch: *mut c_void, scratch_elems: u64, transcript: *const bnh_transcript, products_out: *mut bn_f128, round_proofs_out: *mut bn_f128,
		layer_evals_out: *mut bn_f128, final_points_out: *mut bn_f128, final_evals_out: *mut bn_f128, step_ms_out: *mut f64,
	) -> c_int;
	pub fn bnh_gkr_exp_prove_live(
		ctx: *mut bn_ctx, n_witnesses: u32, widths: *const u32, kinds: *const u32, d_exponent_bits: *const *const c_void, static_bases: *const bn_f128,
		d_bases: *const *const c_void, d_arenas: *const *mut c_void, n_claims: u32, n_vars: *const u32, eval_points: *const bn_f128, evals: *const bn_f128,
		d_scratch: *mut c_void, scratch_elems: u64, transcript: *const bnh_transcript, n_layers_out: *mut u32, rounds_per_layer_out: *mut u32,
		coeffs_per_round_out: *mut u32, round_proofs_out: *mut bn_f128, provers_per_layer_out: *mut u32, evals_per_prover_out: *mut u32,
		multilinear_evals_out: *mut bn_f128, claims_per_layer_out: *mut u32, claim_n_vars_out: *mut u32, claim_points_out: *mut bn_f128, claim_evals_out: *mut bn_f128,
		layer_ms_out: *mut f64,
	) -> c_int;
	pub fn bnh_flush_prodcheck_prove_live(
		ctx: *mut bn_ctx, n_flushes: u32, channel_ids: *const u32, flush_n_vars: *const u32, n_selectors: *const u32, selector_ids: *const u32,
		d_selectors: *const *const c_void, n_entries: *const u32, entry_kinds: *const u32, entry_ids: *const u32, d_entry_columns: *const *const c_void,
		entry_levels: *const u32, entry_consts: *const bn_f128, n_nonzero: u32, nonzero_ids: *const u32, d_nonzero_columns: *const *const c_void,
		nonzero_levels: *const u32, nonzero_n_vars: *const u32, n_channels: u32, d_scratch: *mut c_void, scratch_elems: u64, transcript: *const bnh_transcript,
		prefix_lens_out: *mut u64, products_out: *mut bn_f128, gpa_round_proofs_out: *mut bn_f128, gpa_layer_evals_out: *mut bn_f128,
		gpa_final_points_out: *mut bn_f128, gpa_final_evals_out: *mut bn_f128, n_checks_out: *mut u32, check_desc_out: *mut u32, check_ids_out: *mut u32,
		check_round_proofs_out: *mut bn_f128, check_final_evals_out: *mut bn_f128, n_linear_out: *mut u32, linear_flushes_out: *mut u32, phase_ms_out: *mut f64,
	) -> c_int;
	pub fn bnh_evalcheck_bivariate_prove_lc_live(
		ctx: *mut bn_ctx, n_provers: u32, prover_desc: *const u32, ml_desc: *const u32, d_columns: *const *const c_void, n_terms: u32, term_levels: *const u32,
		d_term_columns: *const *const c_void, term_coeffs: *const bn_f128, ml_offsets: *const bn_f128, point_pool: *const bn_f128, pool_len: u32,
		comp_indices: *const u32, sums: *const bn_f128, d_scratch: *mut c_void, scratch_elems: u64, transcript: *const bnh_transcript, round_proofs_out: *mut bn_f128,
		final_evals_out: *mut bn_f128,
	) -> c_int;
	pub fn bnh_ring_switch_prove_live(
		ctx: *mut bn_ctx, n_columns: u32, d_columns: *const *const c_void, column_desc: *const u32, point_pool: *const bn_f128, pool_len: u32, n_suffixes: u32,
		suffix_desc: *const u32, n_prefixes: u32, prefix_kappas: *const u32, n_claims: u32, claim_desc: *const u32, transcript: *const bnh_transcript,
		d_scratch: *mut c_void, scratch_elems: u64, mixed_tensor_elems_out: *mut bn_f128, row_batched_evals_out: *mut bn_f128, d_transparents_out: *mut *mut c_void,
		phase_ms_out: *mut f64,
	) -> c_int;
	pub fn bnh_fri_prove_live(
		ctx: *mut bn_ctx, log_dim: u32, log_inv_rate: u32, log_batch_size: u32, fold_arities: *const u32, n_arities: u32, n_test_queries: u32,
		d_message: *const c_void, d_scratch: *mut c_void, scratch_elems: u64, transcript: *const bnh_transcript, roots_out: *mut u8, advice_out: *mut bn_f128,
		max_advice_elems: u64, n_advice_elems_out: *mut u64, phase_ms_out: *mut f64,
	) -> c_int;
	pub fn bnh_piop_prove_committed_open_live(
		ctx: *mut bn_ctx, n_committed: u32, committed_n_vars: *const u32, d_committed: *const *const c_void, n_transparent: u32, transparent_n_vars: *const u32,
		d_transparent: *const *const c_void, n_claims: u32, claims: *const u32, claim_sums: *const bn_f128, log_dim: u32, log_inv_rate: u32, log_batch_size: u32,
		fold_arities: *const u32, n_arities: u32, n_test_queries: u32, d_codeword: *const c_void, d_tree: *const c_void, d_scratch: *mut c_void, scratch_elems: u64,
		transcript: *const bnh_transcript, items_out: *mut u32, max_items: u32, n_items_out: *mut u32, scalars_out: *mut bn_f128, max_scalars: u64,
		n_scalars_out: *mut u64, digests_out: *mut u8, max_digests: u32, n_digests_out: *mut u32, phase_ms_out: *mut f64, advice_out: *mut bn_f128,
		max_advice_elems: u64, n_advice_elems_out: *mut u64,
	) -> c_int;
	pub fn bnh_transcript_replay_new(
		samples: *const bn_f128, n_samples: u64, bit_samples: *const u64, n_bit_samples: u64, handle_out: *mut *mut bnh_transcript_replay,
	) -> c_int;
	pub fn bnh_transcript_replay_table(handle: *mut bnh_transcript_replay) -> *const bnh_transcript;
	pub fn bnh_transcript_replay_written(handle: *mut bnh_transcript_replay, channel: u32, buf: *mut u8, max: u64, len_out: *mut u64) -> c_int;
	pub fn bnh_transcript_replay_events(handle: *mut bnh_transcript_replay, kinds_out: *mut u32, counts_out: *mut u64, max_events: u64, n_events_out: *mut u64) -> c_int;
	pub fn bnh_transcript_replay_free(handle: *mut bnh_transcript_replay);

}
