// binius_amd/csrc/abi_expcircuit.cpp -- bn_exp_circuit_layers: every layer of a batch of exponentiation circuits, the witness of the
// GKR exponentiation argument (core/src/protocols/gkr_exp/witness.rs:31-110, 139-156, 258-284), and bn_bits_to_b128, the bit columns
// as B128 multilinears that its prover folds.  Argument validation and the plan of the launch; the kernels are in
// kernels_expcircuit.hip.
//
// The plan: one job per witness, ceil(2^n_vars / 224) units each (a wave takes a unit through all layers), ONE launch for the
// call.  One upload carries the job table, the witnesses' bit-column pointers and, for static bases, the constants g^(2^k)
// (host scalar work: width - 1 squarings per witness).
#include <algorithm>

#include "abi_common.hpp"
#include "hostmul.hpp"

extern "C" {

int bn_exp_circuit_layers(bn_ctx *ctx, uint32_t n_witnesses, const uint32_t *n_vars, const uint32_t *widths, const uint32_t *kinds,
                          const void *const *d_exponent_bits, const bn_f128 *static_bases, const void *const *d_bases, void *const *d_layers)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n_witnesses == 0) return BN_OK;
	BN_REQUIRE(n_vars && widths && kinds && d_exponent_bits && static_bases && d_bases && d_layers, "null argument");
	BN_REQUIRE(n_witnesses <= (1u << 16), "too many witnesses for one call");
	uint64_t units = 0;
	size_t n_ptrs = 0, n_pows = 0;
	for (uint32_t t = 0; t < n_witnesses; t++) {
		BN_REQUIRE(n_vars[t] <= BN_EXP_MAX_VARS, "exp circuit: n_vars out of range (0 .. 28)");
		BN_REQUIRE(widths[t] >= 1 && widths[t] <= BN_EXP_MAX_WIDTH, "exp circuit: width out of range (1 .. 128)");
		BN_REQUIRE(kinds[t] == BN_EXP_STATIC || kinds[t] == BN_EXP_DYNAMIC, "exp circuit: unknown kind");
		const uint64_t rows = (uint64_t)1 << n_vars[t], arena_elems = rows * widths[t];
		BN_REQUIRE(d_layers[t], "exp circuit: null layer arena");
		BN_REQUIRE(aligned16(d_layers[t]), "exp circuit: pointers must be 16-byte aligned");
		for (uint32_t j = 0; j < widths[t]; j++) {
			const void *col = d_exponent_bits[n_ptrs + j];
			BN_REQUIRE(col, "exp circuit: null bit column");
			BN_REQUIRE(aligned16(col), "exp circuit: pointers must be 16-byte aligned");
			BN_REQUIRE(!ranges_overlap(col, column_elems(n_vars[t], 0), d_layers[t], arena_elems), "exp circuit: the layer arena overlaps a bit column");
		}
		if (kinds[t] == BN_EXP_DYNAMIC) {
			BN_REQUIRE(d_bases[t], "exp circuit: null base column");
			BN_REQUIRE(aligned16(d_bases[t]), "exp circuit: pointers must be 16-byte aligned");
			BN_REQUIRE(!ranges_overlap(d_bases[t], rows, d_layers[t], arena_elems), "exp circuit: the layer arena overlaps the base column");
		} else {
			n_pows += widths[t];
		}
		n_ptrs += widths[t];
		units += (rows + bn::kExpRun - 1) / bn::kExpRun;
		BN_REQUIRE(units < (1ull << 31), "exp circuit: batch too large for one call");
	}

	// ---- one upload: [jobs][bit-column pointers][g^(2^k)]
	call_upload up(ctx);
	const auto s_jobs = up.reserve<bn::expc_job>(n_witnesses);
	const auto s_ptrs = up.reserve<const uint32_t *>(n_ptrs);
	const auto s_pows = up.reserve<f128>(n_pows);
	if (const int rc = up.alloc()) return rc;
	bn::expc_job *jobs = up.host(s_jobs);
	f128 *pows = up.host(s_pows);
	memcpy(up.host(s_ptrs), d_exponent_bits, n_ptrs * sizeof(void *));
	size_t at_ptr = 0, at_pow = 0;
	uint32_t at_unit = 0;
	for (uint32_t t = 0; t < n_witnesses; t++) {
		bn::expc_job &jb = jobs[t];
		jb.bits = up.dev(s_ptrs) + at_ptr;
		jb.arena = (f128 *)d_layers[t];
		jb.rows = (uint64_t)1 << n_vars[t];
		jb.width = widths[t];
		jb.dynamic = kinds[t] == BN_EXP_DYNAMIC;
		jb.start = at_unit;
		if (jb.dynamic) {
			jb.base = (const f128 *)d_bases[t];
		} else {
			jb.base = up.dev(s_pows) + at_pow;
			f128 p = to_f(&static_bases[t]);
			for (uint32_t k = 0; k < widths[t]; k++) {
				pows[at_pow + k] = p;
				p = bn::mul_host(p, p);
			}
			at_pow += widths[t];
		}
		at_ptr += widths[t];
		at_unit += (uint32_t)((jb.rows + bn::kExpRun - 1) / bn::kExpRun);
	}
	BN_HIP(up.send());
	BN_HIP(bn::launch_expcircuit(ctx->stream, ctx->n_cu, up.dev(s_jobs), n_witnesses, at_unit));
	ctx->exp_calls++;
	ctx->exp_launches++;
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the layers are complete on return; the table is pageable host memory that goes out of scope)
	return BN_OK;
}

int bn_bits_to_b128(bn_ctx *ctx, uint32_t n, const uint32_t *log_lens, const void *const *d_srcs, void *const *d_dsts)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n == 0) return BN_OK;
	BN_REQUIRE(log_lens && d_srcs && d_dsts, "null argument");
	BN_REQUIRE(n <= (1u << 20), "too many arrays for one call");
	std::vector<bn::bits_job> jobs(n);
	uint64_t blocks = 0;
	for (uint32_t t = 0; t < n; t++) {
		BN_REQUIRE(log_lens[t] <= BN_EXP_MAX_VARS, "bits: log_len out of range (0 .. 28)");
		const uint64_t full = (uint64_t)1 << log_lens[t];
		BN_REQUIRE(d_srcs[t] && d_dsts[t], "bits: null pointer");
		BN_REQUIRE(aligned16(d_srcs[t], d_dsts[t]), "bits: pointers must be 16-byte aligned");
		BN_REQUIRE(!ranges_overlap(d_srcs[t], column_elems(log_lens[t], 0), d_dsts[t], full), "bits: destination overlaps its source");
		jobs[t] = bn::bits_job{(const uint32_t *)d_srcs[t], (f128 *)d_dsts[t], full, (uint32_t)blocks, 0};
		blocks += (full + 255) / 256;
		BN_REQUIRE(blocks < (1ull << 31), "bits: batch too large for one call");
	}
	char *scr = (char *)bn::ctx_scratch(ctx, jobs.size() * sizeof(bn::bits_job));
	if (!scr) return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (scratch)");
	BN_HIP(hipMemcpyAsync(scr, jobs.data(), jobs.size() * sizeof(bn::bits_job), hipMemcpyHostToDevice, ctx->stream));
	BN_HIP(bn::launch_bits_to_b128(ctx->stream, (const bn::bits_job *)scr, n, (uint32_t)blocks));
	ctx->exp_bits_launches++;
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the table is pageable host memory that goes out of scope)
	return BN_OK;
}

int bn_exp_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_EXP_CALLS] = ctx->exp_calls;
	counters[BN_EXP_LAUNCHES] = ctx->exp_launches;
	counters[BN_EXP_BITS_LAUNCHES] = ctx->exp_bits_launches;
	return BN_OK;
}

} // extern "C"
