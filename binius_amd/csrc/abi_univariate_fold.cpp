// binius_amd/csrc/abi_univariate_fold.cpp -- bn_univariate_fold_batch: the fold of the univariate round of the univariate-skip
// zerocheck for every column of a call (ZerocheckProverImpl::fold_univariate_round, core/src/protocols/sumcheck/prove/zerocheck.rs:
// 384-434).  Argument validation and the plan of the launch; the kernel is in kernels_univariate_fold.hip.
//
// The plan: one job per column, sorted by tower level; a job is cut into units of 2048 outputs (512 for rows of 64 bytes and more);
// the launch has at most three workgroups per CU (two when the tables need more than 32 KiB of LDS), each of which takes a contiguous
// range of the units.  One upload carries the coefficients and the job table.
#include <algorithm>

#include "abi_common.hpp"

extern "C" {

int bn_univariate_fold_batch(bn_ctx *ctx, const void *cols_, uint32_t n_cols, uint32_t skip_rounds, const bn_f128 *h_coeffs, void *const *d_outs)
{
	const bn_pe_column *cols = (const bn_pe_column *)cols_;
	const uint32_t k = skip_rounds;
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n_cols == 0) return BN_OK;
	BN_REQUIRE(cols && h_coeffs && d_outs, "null argument");
	BN_REQUIRE(n_cols <= (1u << 20), "too many columns for one call");
	BN_REQUIRE(k >= 1 && k <= BN_UNIVARIATE_FOLD_MAX_SKIP, "univariate fold: skip_rounds out of range (1 .. 8)");
	uint64_t units = 0;
	uint32_t lds_tables = 0;
	for (uint32_t c = 0; c < n_cols; c++) {
		const bn_pe_column &col = cols[c];
		BN_REQUIRE(col.d_evals && d_outs[c], "univariate fold: null pointer");
		BN_REQUIRE(col.tower_level == 0 || col.tower_level == 3, "univariate fold: tower level must be 0 or 3");
		BN_REQUIRE(col.n_vars <= BN_PE_MAX_VARS, "univariate fold: n_vars out of range");
		BN_REQUIRE(k <= col.n_vars, "univariate fold: skip_rounds larger than n_vars");
		BN_REQUIRE(aligned16(col.d_evals, d_outs[c]), "univariate fold: pointers must be 16-byte aligned");
		const uint64_t out_len = (uint64_t)1 << (col.n_vars - k);
		BN_REQUIRE(!ranges_overlap(col.d_evals, column_elems(col.n_vars, col.tower_level), d_outs[c], out_len), "univariate fold: an output overlaps its column");
		const uint64_t unit_rows = 256u * bn::uf_rows_per_thread(k + col.tower_level);
		units += (out_len + unit_rows - 1) / unit_rows;
		BN_REQUIRE(units < (1ull << 31), "univariate fold: batch too large for one call");
		lds_tables = std::max(lds_tables, bn::uf_tables(col.tower_level, k));
	}

	// ---- one upload: [coefficients][jobs], the jobs sorted by level
	std::vector<uint32_t> order(n_cols);
	for (uint32_t c = 0; c < n_cols; c++) order[c] = c;
	std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cols[x].tower_level < cols[y].tower_level; });
	call_upload up(ctx);
	const auto s_coeffs = up.reserve<bn_f128>((size_t)1 << k);
	const auto s_jobs = up.reserve<bn::uf_job>(n_cols);
	if (const int rc = up.alloc()) return rc;
	std::copy(h_coeffs, h_coeffs + ((size_t)1 << k), up.host(s_coeffs));
	bn::uf_job *jobs = up.host(s_jobs);
	uint32_t at_unit = 0;
	for (uint32_t i = 0; i < n_cols; i++) {
		const bn_pe_column &col = cols[order[i]];
		bn::uf_job &jb = jobs[i];
		jb.col = col.d_evals;
		jb.out = (uint4 *)d_outs[order[i]];
		jb.out_len = (uint64_t)1 << (col.n_vars - k);
		jb.level = col.tower_level;
		jb.start = at_unit;
		const uint64_t unit_rows = 256u * bn::uf_rows_per_thread(k + col.tower_level);
		at_unit += (uint32_t)((jb.out_len + unit_rows - 1) / unit_rows);
	}
	const uint32_t per_cu = lds_tables * 256 <= 32768 ? 3 : 2; // (about 160 registers per thread: three workgroups of a CU at most)
	const uint32_t n_wgs = (uint32_t)std::min<uint64_t>(at_unit, (uint64_t)ctx->n_cu * per_cu);
	BN_HIP(up.send());
	BN_HIP(bn::launch_univariate_fold(ctx->stream, up.dev(s_jobs), n_cols, up.dev(s_coeffs), k, at_unit, n_wgs, lds_tables));
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the tables are pageable host memory that goes out of scope; the outputs are complete on return)
	ctx->uf_calls++;
	ctx->uf_launches++;
	ctx->uf_cols += n_cols;
	return BN_OK;
}

int bn_univariate_fold_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_UF_CALLS] = ctx->uf_calls;
	counters[BN_UF_LAUNCHES] = ctx->uf_launches;
	counters[BN_UF_COLS] = ctx->uf_cols;
	return BN_OK;
}

} // extern "C"
