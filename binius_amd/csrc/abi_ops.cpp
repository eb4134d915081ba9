// binius_amd/csrc/abi_ops.cpp -- extern "C" entry points of the executor ops (tensor_expand, inner_product,
// fold_left / fold_right, fri_fold, compute_composite, pairwise_product_reduce), the Merkle / Groestl
// commitment side and the additive NTT: argument validation with the reference's error behaviour, then a
// kernel launch.  No arithmetic fallback lives here.
#include "abi_common.hpp"

namespace bnabi {
// a matrix-core fold that was launched, in the counters of bn_fold_counters
static void count_linmap(uint64_t *counted, int route, int ring2, const bn::linmap_launch &l)
{
	counted[route] += 1;
	if (l.ring_r == 2 || l.ring_r == 4 || l.ring_r == 8) counted[ring2 + (l.ring_r == 2 ? 0 : l.ring_r == 4 ? 1 : 2)] += 1;
	counted[BN_FOLD_LAST_GRID] = l.grid;
	counted[BN_FOLD_LAST_PREP] = l.prep_level;
}

// fold_left on the kernels of kernels_misc.hip / kernels_linmap.hip (arguments validated by the caller)
// counted: the BN_FOLD_* counters of a bn_fold_left call (nullptr: a column of bn_partial_eval_high_batch, which has its own)
int fold_left_dispatch(bn_ctx *ctx, const void *d_mat, uint32_t tower_level, const void *d_vec, uint64_t vec_len, void *d_out, uint64_t out_len,
                       uint64_t *counted)
{
	if (tower_level == 5 && out_len >= 4096 && (vec_len == 16 || vec_len == 32 || vec_len == 64)) {
		void *tab = bn::ctx_scratch(ctx, bn::linmap_table_bytes(vec_len * 32));
		if (tab) {
			bn::linmap_launch l;
			const hipError_t e = bn::launch_fold_left_mfma(ctx->stream, ctx->n_cu, d_mat, tower_level, d_vec, vec_len, d_out, out_len, tab, &l);
			if (e == hipSuccess) {
				if (counted) count_linmap(counted, BN_FOLD_LEFT_MFMA, BN_FOLD_RING_LEFT2, l);
				return BN_OK;
			}
			if (e != hipErrorNotSupported) BN_HIP(e);
		}
	}
	bool by_tab = false;
	BN_HIP(bn::launch_fold_left(ctx->stream, ctx->n_cu, d_mat, tower_level, d_vec, vec_len, d_out, out_len, &by_tab));
	if (counted) counted[by_tab ? BN_FOLD_LEFT_TAB : BN_FOLD_LEFT_SCALAR] += 1;
	return BN_OK;
}
} // namespace bnabi

extern "C" {

int bn_tensor_expand(bn_ctx *ctx, void *d_data, uint64_t data_len, uint32_t log_n, const bn_f128 *h_coords, uint32_t k)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(log_n + k < 64 && data_len == ((uint64_t)1 << (log_n + k)), "invalid data length");
	prof_scope ps(ctx, BN_PROF_TENSOR_EXPAND);
	std::vector<f128> coords(k);
	for (uint32_t i = 0; i < k; i++) coords[i] = to_f(&h_coords[i]);
	BN_HIP(bn::launch_tensor_expand(ctx->stream, ctx->n_cu, d_data, log_n, coords.data(), k));
	return BN_OK;
}

int bn_inner_product(bn_ctx *ctx, const void *d_a, uint64_t a_len, uint32_t tower_level, const void *d_b, uint64_t b_len,
                     bn_f128 *h_out)
{
	BN_REQUIRE(ctx && h_out, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(tower_level <= 7 && (a_len << (7 - tower_level)) == b_len, "invalid input: inner_product lengths");
	BN_REQUIRE(valid_tower_level(tower_level), "unsupported value of tower_level");
	ctx->s_clean = false; // slots 0..1 of the accumulator area are used as this op's accumulators
	BN_HIP(hipMemsetAsync(ctx->d_result, 0, 2 * sizeof(f128), ctx->stream));
	if (tower_level == 7 && b_len >= 2 && (b_len & 1) == 0) {
		// F x F: a plain sum of products -> the bit-sliced product-sum kernel (two half-range streams)
		const bool mfma = bn::mfma_applies(ctx->n_cu, b_len / 2);
		if (mfma)
			BN_HIP(bn::launch_roundeval_mfma_split(ctx->stream, ctx->n_cu, d_a, d_b, b_len / 2, b_len / 2, ctx->d_result));
		else
			BN_HIP(bn::launch_roundeval9_split(ctx->stream, ctx->n_cu, d_a, d_b, b_len / 2, b_len / 2, ctx->d_result));
		ctx->ip_calls[mfma ? BN_IP_MFMA_SPLIT : BN_IP_SPLIT9] += 1;
		return publish_result(ctx, 2, h_out);
	}
	if (tower_level == 5 && b_len >= 8192 && b_len % 512 == 0) {
		// B32 x F: four independent bit-sliced GF(2^32) inner products (kernels_ip32.hip)
		BN_HIP(bn::launch_ip32(ctx->stream, ctx->n_cu, d_a, d_b, b_len, ctx->d_result));
		ctx->ip_calls[BN_IP_IP32] += 1;
		return publish_result(ctx, 1, h_out);
	}
	BN_HIP(bn::launch_inner_product(ctx->stream, ctx->n_cu, d_a, tower_level, d_b, b_len, ctx->d_result));
	ctx->ip_calls[BN_IP_SCALAR] += 1;
	return publish_result(ctx, 1, h_out);
}

int bn_inner_product_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	for (int i = 0; i < BN_IP_N; i++) counters[i] = ctx->ip_calls[i];
	return BN_OK;
}

static int fold_common(bn_ctx *ctx, bool left, const void *d_mat, uint64_t mat_len, uint32_t tower_level, const void *d_vec,
                       uint64_t vec_len, void *d_out, uint64_t out_len)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(tower_level <= 7, "invalid evals: tower_level > 7");
	BN_REQUIRE(valid_tower_level(tower_level), "unsupported value of tower_level");
	BN_REQUIRE(is_pow2(mat_len) && is_pow2(vec_len), "lengths must be powers of two");
	const uint32_t log_evals = ilog2(mat_len) + 7 - tower_level;
	const uint32_t log_q = ilog2(vec_len);
	BN_REQUIRE(log_q <= log_evals, "query larger than evals");
	BN_REQUIRE(out_len == ((uint64_t)1 << (log_evals - log_q)), "output has the wrong number of elements");
	if (left) {
		// few outputs under a long reduction (evaluate_partial_high at evalcheck's shapes): the reduction is split across
		// workgroups by the partial-evaluation kernel, as a one-column job (abi_partial_eval.cpp)
		// (BN_FOLD_LEFT_NO_PE=1, read per call: the fold_left kernels at these shapes too -- the baseline leg of tools/bench_evalcheck.py)
		const char *no_pe = std::getenv("BN_FOLD_LEFT_NO_PE");
		if (out_len <= ((uint64_t)1 << bn::kPeMaxLogOut) && vec_len >= 4096 && !(no_pe && no_pe[0] == '1')) {
			const bn_pe_column col{d_mat, tower_level, log_evals};
			void *const out = d_out;
			const int rc = partial_eval_run(ctx, &col, 1, d_vec, log_q, &out, /*routed=*/true);
			if (rc == BN_OK) ctx->fold_calls[BN_FOLD_LEFT_PE] += 1;
			return rc;
		}
		return fold_left_dispatch(ctx, d_mat, tower_level, d_vec, vec_len, d_out, out_len, ctx->fold_calls);
	}
	// rows of 512 .. 2048 bits: the linear map on the matrix cores (kernels_linmap.hip); every other shape: nibble tables
	const uint64_t row_bits = vec_len << tower_level;
	if (out_len >= 4096 && (row_bits == 512 || row_bits == 1024 || row_bits == 2048)) {
		void *tab = bn::ctx_scratch(ctx, bn::linmap_table_bytes(row_bits));
		if (tab) {
			bn::linmap_launch l;
			const hipError_t e = bn::launch_fold_right_mfma(ctx->stream, ctx->n_cu, d_mat, tower_level, d_vec, vec_len, d_out, out_len, tab, &l);
			if (e == hipSuccess) {
				bnabi::count_linmap(ctx->fold_calls, BN_FOLD_RIGHT_MFMA, BN_FOLD_RING2, l);
				return BN_OK;
			}
			if (e != hipErrorNotSupported) BN_HIP(e);
		}
	}
	bool by_tab = false;
	BN_HIP(bn::launch_fold_right(ctx->stream, ctx->n_cu, d_mat, tower_level, d_vec, vec_len, d_out, out_len, &by_tab));
	ctx->fold_calls[by_tab ? BN_FOLD_RIGHT_TAB : BN_FOLD_RIGHT_SCALAR] += 1;
	return BN_OK;
}

int bn_fold_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	for (int i = 0; i < BN_FOLD_N; i++) counters[i] = ctx->fold_calls[i];
	counters[BN_FOLD_N_CU] = (uint64_t)ctx->n_cu;
	return BN_OK;
}

int bn_fold_left(bn_ctx *ctx, const void *d_mat, uint64_t mat_len, uint32_t tower_level, const void *d_vec, uint64_t vec_len,
                 void *d_out, uint64_t out_len)
{
	return fold_common(ctx, true, d_mat, mat_len, tower_level, d_vec, vec_len, d_out, out_len);
}

int bn_fold_right(bn_ctx *ctx, const void *d_mat, uint64_t mat_len, uint32_t tower_level, const void *d_vec, uint64_t vec_len,
                  void *d_out, uint64_t out_len)
{
	return fold_common(ctx, false, d_mat, mat_len, tower_level, d_vec, vec_len, d_out, out_len);
}

// The twiddle basis of the caller's NTT instance on the device (d_out) + `extra_bytes` of scratch (extra).  The basis is
// caller-owned pageable memory that does not change between the calls of one instance: it is compared with the copy of the
// last call (8 KiB) and uploaded -- one synchronisation -- only when it differs.
static int upload_s_evals(bn_ctx *ctx, const uint64_t *h_s_evals, uint64_t **d_out, size_t extra_bytes, void **extra)
{
	constexpr size_t words = (size_t)BN_NTT_MAX_DIM * BN_NTT_MAX_DIM;
	if (ctx->h_s_evals.size() != words || memcmp(ctx->h_s_evals.data(), h_s_evals, words * sizeof(uint64_t)) != 0) {
		// (kernels of earlier calls that still read the old basis are ahead of the copy on the same stream)
		// (the host copy only names what IS on the device: forgotten first, so that a failed upload is retried by the next call)
		ctx->h_s_evals.clear();
		BN_HIP(hipMemcpyAsync(ctx->d_s_evals, h_s_evals, words * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
		BN_HIP(hipStreamSynchronize(ctx->stream)); // (the source is pageable: the runtime may still be reading it)
		ctx->h_s_evals.assign(h_s_evals, h_s_evals + words);
	}
	*d_out = ctx->d_s_evals;
	if (extra) {
		char *scr = (char *)bn::ctx_scratch(ctx, extra_bytes);
		if (!scr)
			return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (scratch)");
		*extra = scr;
	}
	return BN_OK;
}

int bn_fri_fold(bn_ctx *ctx, const uint64_t *h_s_evals, uint32_t tw_level, uint32_t log_domain, uint32_t log_len,
                uint32_t log_batch_size, const bn_f128 *h_challenges, uint32_t n_challenges, const void *d_in, uint64_t in_len,
                void *d_out, uint64_t out_len)
{
	BN_REQUIRE(ctx && h_s_evals, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH_FOR(ctx, bn_range{d_in, in_len}, bn_range{d_out, out_len}); // (deferred folds of a batch's provers that touch neither stay deferred)
	BN_REQUIRE(log_len + log_batch_size < 64 && in_len == ((uint64_t)1 << (log_len + log_batch_size)), "invalid data_in length");
	BN_REQUIRE(n_challenges >= log_batch_size, "invalid challenges length");
	BN_REQUIRE(n_challenges <= log_batch_size + log_len, "challenges length too big");
	BN_REQUIRE(out_len == ((uint64_t)1 << (log_len - (n_challenges - log_batch_size))), "invalid data_out length");
	BN_REQUIRE(tw_level >= 3 && tw_level <= 6, "unsupported twiddle field");
	BN_REQUIRE(log_len <= log_domain && log_domain <= BN_NTT_MAX_DIM, "NTT domain too small");
	if (n_challenges == 0) {
		BN_HIP(hipMemcpyAsync(d_out, d_in, in_len * sizeof(f128), hipMemcpyDeviceToDevice, ctx->stream));
		ctx->fri_passes[BN_FRI_COPIES] += 1;
		return BN_OK;
	}
	uint64_t *d_s = nullptr;
	void *pp = nullptr;
	int rc = upload_s_evals(ctx, h_s_evals, &d_s, in_len * sizeof(f128), &pp);
	if (rc) return rc;
	std::vector<f128> ch(n_challenges);
	for (uint32_t i = 0; i < n_challenges; i++) ch[i] = to_f(&h_challenges[i]);
	BN_HIP(bn::launch_fri_fold(ctx->stream, d_s, tw_level, log_domain, log_len, log_batch_size, ch.data(), n_challenges, d_in,
	                           d_out, out_len, pp, ctx->n_cu, ctx->d_mul8, ctx->fri_passes));
	return BN_OK;
}

int bn_fri_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	for (int i = 0; i < BN_FRI_N; i++) counters[i] = ctx->fri_passes[i];
	return BN_OK;
}

} // extern "C"

namespace bnabi {
// the device copy of a tower expression's program: ops, constants, input levels, each section 16-byte aligned (made once)
static size_t tower_consts_off(const bn::ct_program &p) { return p.ops.size() * sizeof(bn::ct_op); }
static size_t tower_levels_off(const bn::ct_program &p) { return tower_consts_off(p) + p.consts.size() * sizeof(f128); }
static int ensure_d_tower(bn_ctx *ctx, const bn_expr *e)
{
	if (e->d_tower) return BN_OK;
	const bn::ct_program &p = *e->tower;
	std::vector<char> img(tower_levels_off(p) + (p.input_levels.size() + 4) * sizeof(uint32_t), 0);
	if (!p.ops.empty()) std::memcpy(img.data(), p.ops.data(), p.ops.size() * sizeof(bn::ct_op));
	if (!p.consts.empty()) std::memcpy(img.data() + tower_consts_off(p), p.consts.data(), p.consts.size() * sizeof(f128));
	if (!p.input_levels.empty()) std::memcpy(img.data() + tower_levels_off(p), p.input_levels.data(), p.input_levels.size() * sizeof(uint32_t));
	void *d = nullptr;
	hipError_t err = hipMalloc(&d, img.size());
	if (err != hipSuccess) return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (tower expression)");
	err = hipMemcpyAsync(d, img.data(), img.size(), hipMemcpyHostToDevice, ctx->stream);
	if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream); // (the source is pageable and goes away)
	if (err != hipSuccess) {
		hipFree(d);
		return bn::hip_fail(err, "bn_expr upload");
	}
	e->d_tower = d;
	return BN_OK;
}

// bn_compute_composite with an expression of bn_expr_compile_tower: packed subfield rows, ONE launch of kernels_compose_tower.hip
static int compute_composite_tower(bn_ctx *ctx, const void *const *d_rows, uint32_t n_rows, uint64_t row_len, void *d_out, uint64_t out_len, const bn_expr *expr)
{
	const bn::ct_program &p = *expr->tower;
	const uint32_t L = p.out_level, n_inputs = (uint32_t)p.input_levels.size();
	BN_REQUIRE(d_rows && d_out, "null argument");
	BN_REQUIRE(row_len == out_len, "inputs and output must be the same length");
	BN_REQUIRE(n_inputs <= n_rows, "composition not match with input");
	BN_REQUIRE(is_pow2(row_len) && ilog2(row_len) <= BN_PE_MAX_VARS && ilog2(row_len) + L >= 7, "the number of values is no power of two, or the output is below one element");
	const uint32_t n_vars = ilog2(row_len);
	const uint64_t out_elems = column_elems(n_vars, L);
	BN_REQUIRE(aligned16(d_out), "misaligned pointer");
	for (uint32_t v = 0; v < n_inputs; v++) {
		BN_REQUIRE(d_rows[v] && aligned16(d_rows[v]), "null or misaligned row");
		BN_REQUIRE(!ranges_overlap(d_out, out_elems, d_rows[v], column_elems(n_vars, p.input_levels[v])), "the output overlaps a row");
	}
	BN_REQUIRE(ctx->device == expr->device, "the expression was compiled for another device");
	const void **d_ptrs = nullptr;
	int rc = ensure_d_tower(ctx, expr);
	if (rc) return rc;
	rc = upload_ptrs(ctx, d_rows, n_inputs, &d_ptrs);
	if (rc) return rc;
	bn::compose_tower_args a{};
	a.rows = d_ptrs;
	a.ops = expr->d_tower;
	a.consts = (const char *)expr->d_tower + tower_consts_off(p);
	a.in_levels = (const uint32_t *)((const char *)expr->d_tower + tower_levels_off(p));
	a.n_ops = (uint32_t)p.ops.size();
	a.result = p.result;
	a.out_level = L;
	a.out_elems = out_elems;
	a.out = d_out;
	BN_HIP(bn::launch_compose_tower(ctx->stream, a, p.n_slots));
	ctx->cc_tower[BN_CC_TOWER_CALLS] += 1;
	ctx->cc_tower[BN_CC_TOWER_LAUNCHES] += 1;
	ctx->cc_tower[L == 0 ? BN_CC_TOWER_BITWISE : BN_CC_TOWER_VALUES] += 1;
	return BN_OK;
}

// bn_compute_composite with a batch of bn_expr_compile_tower_batch: d_out is the arena, one upload
// [job table][ops][constants][input levels][row pointers], ONE launch of k_compose_tower_batch
static int compute_composite_tower_batch(bn_ctx *ctx, const void *const *d_rows, uint32_t n_rows, uint64_t row_len, void *d_out, uint64_t out_len, const bn_expr *expr)
{
	const bn::compose_batch_plan &p = *expr->tower_batch;
	BN_REQUIRE(d_rows && d_out, "null argument");
	BN_REQUIRE(ctx->device == expr->device, "the expression was compiled for another device");
	static_assert(sizeof(uint64_t) == sizeof(const void *), "row pointers are read as addresses");
	const char *why = bn::cb_check_call(p, (const uint64_t *)d_rows, n_rows, row_len, (uint64_t)(uintptr_t)d_out, out_len);
	if (why) return bn::fail(BN_ERR_INPUT_VALIDATION, std::string("input validation: tower batch: ") + why);
	call_upload up(ctx);
	const auto s_jobs = up.reserve<bn::compose_batch_job>(p.jobs.size());
	const auto s_ops = up.reserve<bn::ct_op>(p.n_ops);
	const auto s_consts = up.reserve<f128>(p.n_consts);
	const auto s_levels = up.reserve<uint32_t>(p.n_levels);
	const auto s_rows = up.reserve<const void *>(p.n_rows);
	if (const int rc = up.alloc()) return rc;
	std::copy(p.jobs.begin(), p.jobs.end(), up.host(s_jobs));
	bn::cb_fill(p, up.host(s_ops), up.host(s_consts), up.host(s_levels));
	std::copy(d_rows, d_rows + p.n_rows, up.host(s_rows));
	BN_HIP(up.send());
	bn::compose_batch_args a{};
	a.jobs = up.dev(s_jobs);
	a.ops = up.dev(s_ops);
	a.consts = up.dev(s_consts);
	a.in_levels = up.dev(s_levels);
	a.rows = up.dev(s_rows);
	a.out = d_out;
	a.n_jobs = (uint32_t)p.jobs.size();
	BN_HIP(bn::launch_compose_tower_batch(ctx->stream, a, p.total_units, p.lds_bytes));
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the tables are pageable host memory that goes out of scope)
	ctx->cc_batch[BN_CCB_CALLS] += 1;
	ctx->cc_batch[BN_CCB_LAUNCHES] += 1;
	ctx->cc_batch[BN_CCB_JOBS] += p.jobs.size();
	ctx->cc_batch[BN_CCB_PROGRAMS] += p.programs.size();
	return BN_OK;
}
} // namespace bnabi

extern "C" {

int bn_compute_composite_batch_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	for (int i = 0; i < BN_CCB_N; i++) counters[i] = ctx->cc_batch[i];
	return BN_OK;
}

int bn_compute_composite_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	for (int i = 0; i < BN_CC_N; i++) counters[i] = ctx->cc_tower[i];
	return BN_OK;
}

// rows -> device array of row pointers, staged in the tail of the result mailbox area
int bn_compute_composite(bn_ctx *ctx, const void *const *d_rows, uint32_t n_rows, uint64_t row_len, void *d_out,
                         uint64_t out_len, const bn_expr *expr)
{
	BN_REQUIRE(ctx && expr, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (expr->is_tower_batch()) return compute_composite_tower_batch(ctx, d_rows, n_rows, row_len, d_out, out_len, expr);
	if (expr->is_tower()) return compute_composite_tower(ctx, d_rows, n_rows, row_len, d_out, out_len, expr);
	BN_REQUIRE(row_len == out_len, "inputs and output must be the same length");
	BN_REQUIRE(expr->n_vars == n_rows || (expr->n_vars <= n_rows), "composition not match with input");
	BN_REQUIRE(expr->steps.size() <= 64, "circuit too large for this backend (max 64 steps)");
	if (expr->shape == bn_expr::PRODUCT && expr->product_vars.size() == 2) {
		BN_HIP(bn::launch_mul9(ctx->stream, ctx->n_cu, d_rows[expr->product_vars[0]], 1, d_rows[expr->product_vars[1]], 1, 0, d_out,
		                       row_len));
		return BN_OK;
	}
	int rc;
	if (circuit_multipass_applies(ctx, expr, row_len)) {
		// any other circuit: compiled into passes of the throughput kernels (abi_circuit.cpp)
		rc = circuit_multipass_map(ctx, expr, d_rows, row_len, d_out, 0);
		if (rc != kCircuitDeclined) return rc;
	}
	const void **d_ptrs = nullptr;
	rc = upload_ptrs(ctx, d_rows, n_rows, &d_ptrs);
	if (rc) return rc;
	rc = ensure_d_steps(expr);
	if (rc) return rc;
	BN_HIP(bn::launch_compute_composite_generic(ctx->stream, d_ptrs, n_rows, row_len, d_out, expr->d_steps,
	                                            (uint32_t)expr->steps.size()));
	return BN_OK;
}

int bn_pairwise_product_reduce(bn_ctx *ctx, const void *d_in, uint64_t n, void *const *d_round_outs, const uint64_t *round_lens,
                               uint32_t n_rounds)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(is_pow2(n), "input length must be a power of 2");
	BN_REQUIRE(n >= 2, "input length must be greater than or equal to 2 in order to perform at least one reduction");
	const uint32_t log_n = ilog2(n);
	BN_REQUIRE(n_rounds == log_n, "round_outputs.len() does not match the expected length");
	for (uint32_t r = 0; r < n_rounds; r++)
		BN_REQUIRE(round_lens[r] == ((uint64_t)1 << (log_n - r - 1)), "round_outputs[i].len() has the wrong size");
	// Large levels: the element-wise product (kernels_mul9.hip, at throughput), up to BN_MUL9_FUSE (2) levels per launch
	// (k_mul9_tree: a workgroup goes on with the products under the 896 it has just stored).  From 2^15 elements down a
	// level is one dependent chain whatever its size, and the tree is walked by workgroups that keep their subtree on the CU
	// (kernels_pairtree.hip): up to BN_PAIRTREE_LOG_S (6) levels per launch.  (Round 2 measured the bit-sliced product itself inside one
	// workgroup for the last 12 levels: 233 vs 225 us -- its chain is the cost)
	static const uint32_t tree_max_log2 = [] {
		const char *e = bn::settled_knob("BN_PAIRTREE_MAX_LOG2"); // measurement knob: 0 = off
		const int v = e ? atoi(e) : 15;
		return (uint32_t)(v < 0 ? 0 : (v > 24 ? 24 : v));
	}();
	static const uint32_t tree_log_s = [] {
		const char *e = bn::settled_knob("BN_PAIRTREE_LOG_S");
		const int v = e ? atoi(e) : 6;
		return (uint32_t)(v < 1 ? 1 : (v > 8 ? 8 : v));
	}();
	const void *src = d_in;
	uint32_t r = 0;
	static const uint32_t fuse = [] {
		const char *e = bn::settled_knob("BN_MUL9_FUSE"); // levels per launch of the element-wise kernel (1 .. 4)
		const int v = e ? atoi(e) : 2;
		return (uint32_t)(v < 1 ? 1 : (v > 4 ? 4 : v));
	}();
	while (r < n_rounds && log_n - r > tree_max_log2) {
		uint32_t k = log_n - r - tree_max_log2; // levels left for this kernel
		if (k > fuse) k = fuse;
		if (k == 1) {
			BN_HIP(bn::launch_mul9(ctx->stream, ctx->n_cu, src, 2, src, 2, 1, d_round_outs[r], round_lens[r]));
		} else {
			bn::mul9_tree_args ta{};
			ta.in = (const uint32_t *)src;
			ta.n0 = round_lens[r];
			ta.n_levels = k;
			for (uint32_t l = 0; l < k; l++) ta.lv[l] = (uint32_t *)d_round_outs[r + l];
			BN_HIP(bn::launch_mul9_tree(ctx->stream, ctx->n_cu, ta));
		}
		r += k;
		src = d_round_outs[r - 1];
	}
	while (r < n_rounds) {
		const uint32_t log_m = log_n - r; // elements of `src`
		const uint32_t nl = log_m < tree_log_s ? log_m : tree_log_s;
		bn::pairtree_args pa{};
		pa.in = (const f128 *)src;
		pa.n_levels = nl;
		for (uint32_t l = 0; l < nl; l++) pa.out[l] = (f128 *)d_round_outs[r + l];
		BN_HIP(bn::launch_pairtree(ctx->stream, pa, tree_log_s, (uint64_t)1 << (log_m - nl)));
		r += nl;
		src = d_round_outs[r - 1];
	}
	return BN_OK;
}

// ---------------------------------------------------------------------------------- Merkle / Groestl
int bn_groestl256_leaves(bn_ctx *ctx, const void *d_elems, uint64_t n_elems, uint64_t batch_size, void *d_digests)
{
	BN_REQUIRE(ctx && d_elems && d_digests, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(batch_size != 0 && n_elems % batch_size == 0, "IncorrectBatchSize");
	BN_HIP(bn::launch_groestl_leaves(ctx->stream, ctx->n_cu, d_elems, batch_size, n_elems / batch_size, d_digests));
	return BN_OK;
}

int bn_groestl256_compress_layer(bn_ctx *ctx, const void *d_prev, uint64_t n_out, void *d_next)
{
	BN_REQUIRE(ctx && d_prev && d_next, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_HIP(bn::launch_groestl_layer(ctx->stream, ctx->n_cu, d_prev, n_out, d_next));
	return BN_OK;
}

int bn_merkle_build(bn_ctx *ctx, const void *d_elems, uint64_t n_elems, uint64_t batch_size, void *d_nodes)
{
	BN_REQUIRE(ctx && d_elems && d_nodes, "null argument");
	BN_ENTER(ctx);
	BN_REQUIRE(batch_size != 0 && n_elems % batch_size == 0, "IncorrectBatchSize");
	BN_FLUSH_FOR(ctx, bn_range{d_elems, n_elems}, bn_range{d_nodes, 2 * (2 * (n_elems / batch_size) - 1)});
	const uint64_t n_leaves = n_elems / batch_size;
	BN_REQUIRE(n_leaves != 0 && (n_leaves & (n_leaves - 1)) == 0, "PowerOfTwoLengthRequired");
	BN_HIP(bn::launch_groestl_leaves(ctx->stream, ctx->n_cu, d_elems, batch_size, n_leaves, d_nodes));
	BN_HIP(bn::launch_merkle_layers(ctx->stream, ctx->n_cu, d_nodes, n_leaves));
	return BN_OK;
}

// Openings: h_out[i * item_elems .. +item_elems) = d_src[h_offsets[i] .. +item_elems).  One kernel reads the
// offsets from and writes the items to pinned host memory; one synchronisation.
int bn_gather_d2h(bn_ctx *ctx, const void *d_src, const uint64_t *h_offsets, uint64_t n_items, uint64_t item_elems, bn_f128 *h_out)
{
	BN_REQUIRE(ctx && d_src && (n_items == 0 || (h_offsets && h_out)), "null argument");
	BN_ENTER(ctx);
	{
		uint64_t hi = 0; // (the items lie inside [d_src, d_src + max offset + item_elems))
		for (uint64_t i = 0; i < n_items; i++)
			if (h_offsets[i] > hi) hi = h_offsets[i];
		BN_FLUSH_FOR(ctx, bn_range{d_src, hi + item_elems});
	}
	if (n_items == 0 || item_elems == 0) return BN_OK;
	BN_REQUIRE(n_items <= (1ull << 24) && item_elems <= (1ull << 24) && n_items * item_elems <= (1ull << 26), "gather: too many elements for one call");
	if (n_items == 1 && item_elems <= 64) {
		// one short item -- the root of a tree just built (MerkleTreeProver::commit reads it every FRI commit round,
		// fri/prove.rs:395-420): through the zero-copy mailbox, a spin on the sequence word instead of a stream synchronisation
		// (flush_for_ranges above left no mirrored fold in the mailbox)
		f128 vals[64];
		const int rc = publish_vals(ctx, (const f128 *)d_src + h_offsets[0], 1, (uint32_t)item_elems, 0, 1, vals);
		if (rc) return rc;
		for (uint64_t e = 0; e < item_elems; e++) h_out[e] = bn_f128{vals[e].lo, vals[e].hi};
		return BN_OK;
	}
	const size_t off_bytes = ((size_t)n_items * 8 + 15) & ~(size_t)15;
	const size_t need = off_bytes + (size_t)n_items * item_elems * sizeof(f128);
	if (need > ctx->gather_bytes) {
		BN_HIP(hipStreamSynchronize(ctx->stream));
		if (ctx->h_gather) hipHostFree(ctx->h_gather);
		ctx->h_gather = nullptr;
		ctx->gather_bytes = 0;
		size_t cap = 1 << 16;
		while (cap < need) cap <<= 1;
		if (hipHostMalloc(&ctx->h_gather, cap, hipHostMallocMapped) != hipSuccess)
			return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (pinned gather buffer)");
		BN_HIP(hipHostGetDevicePointer(&ctx->d_gather, ctx->h_gather, 0));
		ctx->gather_bytes = cap;
	}
	std::memcpy(ctx->h_gather, h_offsets, (size_t)n_items * 8);
	BN_HIP(bn::launch_gather(ctx->stream, d_src, (const uint64_t *)ctx->d_gather, n_items, item_elems, (char *)ctx->d_gather + off_bytes));
	BN_HIP(hipStreamSynchronize(ctx->stream));
	std::memcpy(h_out, (const char *)ctx->h_gather + off_bytes, (size_t)n_items * item_elems * sizeof(f128));
	return BN_OK;
}

// ---------------------------------------------------------------------------------- NTT
static int ntt_common(bn_ctx *ctx, bool inverse, void *d_data, uint32_t elem_level, uint32_t tw_level,
                      const uint64_t *h_s_evals, uint32_t log_domain, uint32_t log_x, uint32_t log_y, uint32_t log_z,
                      uint64_t coset, uint32_t coset_bits, uint32_t skip_rounds)
{
	BN_REQUIRE(ctx && h_s_evals, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(elem_level >= 3 && elem_level <= 7, "unsupported element field");
	BN_REQUIRE(tw_level >= 3 && tw_level <= 6 && tw_level <= elem_level, "unsupported twiddle field");
	BN_REQUIRE(log_domain >= 1 && log_domain <= BN_NTT_MAX_DIM && log_domain <= (1u << tw_level), "bad NTT domain");
	BN_REQUIRE(coset_bits >= 64 || coset < ((uint64_t)1 << coset_bits), "coset index out of bounds");
	BN_REQUIRE(log_y + coset_bits <= log_domain, "NTT domain too small");
	BN_REQUIRE(skip_rounds <= log_y, "skip_rounds larger than log_y");
	BN_REQUIRE(log_x + log_y + log_z < 48, "transform too large");
	if (log_y == 0 || skip_rounds == log_y) return BN_OK;
	if (elem_level >= 5 && tw_level == 5 && log_y >= 14 && !bn::settled_knob("BN_NTT_NO_BITSLICE")) {
		// large transforms with B32 twiddles: bit-sliced butterflies (kernels_ntt_bs.hip); B64 / B128
		// data and log_x / log_z batches are interleaved B32 transforms
		const uint32_t lx = log_x + (elem_level - 5);
		void *scr = bn::ctx_scratch(ctx, bn::ntt_bs_scratch_bytes(log_y + lx + log_z));
		if (!scr) return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (NTT scratch)");
		if (!ctx->ntt_cache) {
			bn::ntt_bs_cache *nc = new bn::ntt_bs_cache;
			if (hipMalloc(&nc->d_tables, bn::ntt_bs_tables_bytes()) != hipSuccess) {
				delete nc;
				return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (NTT tables)");
			}
			ctx->ntt_cache = nc;
		}
		prof_scope ps(ctx, BN_PROF_NTT);
		hipError_t be = bn::launch_ntt_bs(ctx->stream, inverse, d_data, h_s_evals, log_domain, lx, log_y, log_z, coset, coset_bits,
		                                  skip_rounds, scr, (bn::ntt_bs_cache *)ctx->ntt_cache);
		if (be == hipSuccess) {
			ctx->ntt_calls_bs++;
			return BN_OK;
		}
		if (be != hipErrorNotSupported) return bn::hip_fail(be, "launch_ntt_bs");
	}
	uint64_t *d_s = nullptr;
	int rc = upload_s_evals(ctx, h_s_evals, &d_s, 0, nullptr);
	if (rc) return rc;
	prof_scope ps(ctx, BN_PROF_NTT);
	if (!bn::settled_knob("BN_NTT_PER_LAYER")) {
		hipError_t te = bn::launch_ntt_tiled(ctx->stream, ctx->n_cu, inverse, d_data, elem_level, tw_level, ctx->d_mul8, d_s, log_domain,
		                                     log_x, log_y, log_z, coset, coset_bits, skip_rounds);
		if (te == hipSuccess) {
			ctx->ntt_calls_tiled++;
			return BN_OK;
		}
		if (te != hipErrorNotSupported) return bn::hip_fail(te, "launch_ntt_tiled");
	}
	BN_HIP(bn::launch_ntt(ctx->stream, inverse, d_data, elem_level, tw_level, d_s, log_domain, log_x, log_y, log_z, coset,
	                      coset_bits, skip_rounds));
	ctx->ntt_calls_layer++;
	return BN_OK;
}

int bn_ntt_forward(bn_ctx *ctx, void *d_data, uint32_t elem_level, uint32_t tw_level, const uint64_t *h_s_evals,
                   uint32_t log_domain, uint32_t log_x, uint32_t log_y, uint32_t log_z, uint64_t coset, uint32_t coset_bits,
                   uint32_t skip_rounds)
{
	return ntt_common(ctx, false, d_data, elem_level, tw_level, h_s_evals, log_domain, log_x, log_y, log_z, coset, coset_bits,
	                  skip_rounds);
}

int bn_ntt_inverse(bn_ctx *ctx, void *d_data, uint32_t elem_level, uint32_t tw_level, const uint64_t *h_s_evals,
                   uint32_t log_domain, uint32_t log_x, uint32_t log_y, uint32_t log_z, uint64_t coset, uint32_t coset_bits,
                   uint32_t skip_rounds)
{
	return ntt_common(ctx, true, d_data, elem_level, tw_level, h_s_evals, log_domain, log_x, log_y, log_z, coset, coset_bits,
	                  skip_rounds);
}

int bn_ntt_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_NTT_CALLS_BS] = ctx->ntt_calls_bs;
	counters[BN_NTT_CALLS_TILED] = ctx->ntt_calls_tiled;
	counters[BN_NTT_CALLS_LAYER] = ctx->ntt_calls_layer;
	return BN_OK;
}

// OnTheFlyTwiddleAccess::generate over BinarySubspace::with_dim(log_domain)
// (crates/ntt/src/twiddle.rs:107-124, 244-306; crates/math/src/binary_subspace.rs:33-38).
// O(log_domain^2) field operations of host metadata; uses the same gf128.hpp arithmetic as the
// kernels (subfield elements embed into the low bits).
int bn_ntt_s_evals(uint32_t tw_level, uint32_t log_domain, uint64_t *h_s_evals)
{
	BN_REQUIRE(h_s_evals, "null argument");
	BN_REQUIRE(tw_level >= 3 && tw_level <= 6, "unsupported twiddle field");
	BN_REQUIRE(log_domain >= 1 && log_domain <= BN_NTT_MAX_DIM && log_domain <= (1u << tw_level), "bad NTT domain");
	auto mul = [](uint64_t a, uint64_t b) { return bn::mul_slow(f128{a, 0}, f128{b, 0}).lo; };
	const uint32_t bits = 1u << tw_level;
	auto inv = [&](uint64_t a) {
		// a^(2^bits - 2) by square-and-multiply: prod_{i=1}^{bits-1} a^(2^i)
		uint64_t r = 1, sq = a;
		for (uint32_t i = 1; i < bits; i++) {
			sq = mul(sq, sq);
			r = mul(r, sq);
		}
		return r;
	};
	auto subspace_map = [&](uint64_t e, uint64_t c) { return mul(e, e) ^ mul(c, e); };
	const uint32_t d = log_domain;
	std::memset(h_s_evals, 0, sizeof(uint64_t) * BN_NTT_MAX_DIM * BN_NTT_MAX_DIM);
	std::vector<uint64_t> norm(d);
	norm[0] = 1;
	for (uint32_t b = 0; b + 1 < d; b++) h_s_evals[b] = 1ull << (b + 1);
	for (uint32_t i = 1; i < d; i++) {
		const uint64_t *prev = &h_s_evals[(i - 1) * BN_NTT_MAX_DIM];
		uint64_t *cur = &h_s_evals[i * BN_NTT_MAX_DIM];
		norm[i] = subspace_map(prev[0], norm[i - 1]);
		for (uint32_t b = 0; b + 1 + i < d; b++) cur[b] = subspace_map(prev[b + 1], norm[i - 1]);
	}
	for (uint32_t i = 0; i < d; i++) {
		const uint64_t iv = inv(norm[i]);
		uint64_t *cur = &h_s_evals[i * BN_NTT_MAX_DIM];
		for (uint32_t b = 0; b + 1 + i < d; b++) cur[b] = mul(cur[b], iv);
	}
	return BN_OK;
}

} // extern "C"
