// binius_amd/csrc/abi_partial_eval.cpp -- bn_partial_eval_high_batch: a batch of columns evaluated at the high coordinates of one
// point, the projection evalcheck makes of every shifted or packed virtual column's inner column (collect_projected_mles,
// core/src/protocols/evalcheck/subclaims.rs:356-439).  Argument validation and the plan of the launch; the kernel is in
// kernels_partial_eval.hip.
//
// The plan: columns with at most 1024 outputs are sorted by class (tower level, b = log2 of the outputs) and cut into groups of
// up to G columns of one class; a unit (one workgroup) is a chunk of 2^log_ch reduction indices j of one group, so the chunk of
// the query is staged once per group.  log_ch starts at 8 KiB of column per unit; G and log_ch shrink while the launch would not
// fill the device (a single column of 2^22 bits still becomes 256 units).  One upload carries the group and column tables; a
// single column travels as kernel arguments.  Wider columns run on the fold_left kernels inside the same call.
#include <algorithm>

#include "abi_common.hpp"

namespace {

uint32_t pe_log_ch(uint32_t level, uint32_t b, uint32_t q, uint32_t shrink)
{
	const uint32_t lo = (level == 0 && b < 6) ? 6 - b : 0; // a 64-bit word of a bit column is not split between units
	const uint32_t row = b + level;                          // log2 of the bits of a row
	uint32_t l = row >= 16 ? 0 : 16 - row;                   // 8 KiB of the column per unit
	l = std::min(l, bn::kPeLogVecChunk);
	l = l > shrink ? l - shrink : 0;
	l = std::max(l, lo);
	return std::min(l, q);
}

} // namespace

namespace bnabi {

int partial_eval_run(bn_ctx *ctx, const bn_pe_column *cols, uint32_t n_cols, const void *d_vec, uint32_t q, void *const *d_outs, bool routed)
{
	// ---- the columns the kernel serves, sorted by class
	std::vector<uint32_t> order, wide;
	for (uint32_t c = 0; c < n_cols; c++) (cols[c].n_vars - q <= bn::kPeMaxLogOut ? order : wide).push_back(c);
	auto key = [&](uint32_t c) { return (cols[c].tower_level << 8) | (cols[c].n_vars - q); };
	std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return key(x) < key(y); });
	uint64_t max_share = 0;
	if (!order.empty()) {
		static const uint32_t cfgs[6][2] = {{8, 0}, {4, 0}, {2, 0}, {1, 0}, {1, 1}, {1, 2}}; // (columns per group, log_ch shrink)
		std::vector<bn::pe_group> groups;
		uint64_t units = 0;
		for (int pick = 0; pick < 6; pick++) {
			const uint32_t G = cfgs[pick][0], shrink = cfgs[pick][1];
			groups.clear();
			units = 0;
			max_share = 0;
			for (size_t at = 0; at < order.size();) {
				size_t end = at;
				while (end < order.size() && end - at < G && key(order[end]) == key(order[at])) end++;
				const bn_pe_column &c0 = cols[order[at]];
				const uint32_t b = c0.n_vars - q, log_ch = pe_log_ch(c0.tower_level, b, q, shrink);
				const uint64_t n_chunks = (uint64_t)1 << (q - log_ch);
				BN_REQUIRE(units + n_chunks < (1ull << 31), "partial eval: batch too large for one call");
				groups.push_back(bn::pe_group{(uint32_t)at, (uint32_t)(end - at), c0.tower_level, b, log_ch, (uint32_t)units});
				units += n_chunks;
				max_share = std::max(max_share, n_chunks);
				at = end;
			}
			if (units >= (uint64_t)ctx->n_cu * 4) break;
		}
		std::vector<bn::pe_col> table(order.size());
		for (size_t i = 0; i < order.size(); i++) {
			const bn_pe_column &c = cols[order[i]];
			table[i] = bn::pe_col{(const uint64_t *)c.d_evals, (uint64_t *)d_outs[order[i]], 1u << (c.n_vars - q), 0};
		}
		// (every group at level 0 -- the keccak case: the instantiation without the subfield products, at the bit path's own occupancy)
		const bool bits_only = cols[order.back()].tower_level == 0; // (sorted by level)
		if (order.size() == 1) {
			BN_HIP(bn::launch_partial_eval(ctx->stream, nullptr, 1, nullptr, 1, groups[0], table[0], d_vec, (uint32_t)units, bits_only));
		} else {
			call_upload up(ctx);
			const auto s_groups = up.reserve<bn::pe_group>(groups.size());
			const auto s_cols = up.reserve<bn::pe_col>(table.size());
			if (const int rc = up.alloc()) return rc;
			std::copy(groups.begin(), groups.end(), up.host(s_groups));
			std::copy(table.begin(), table.end(), up.host(s_cols));
			BN_HIP(up.send());
			BN_HIP(bn::launch_partial_eval(ctx->stream, up.dev(s_groups), (uint32_t)groups.size(), up.dev(s_cols), (uint32_t)table.size(), bn::pe_group{},
			                               bn::pe_col{}, d_vec, (uint32_t)units, bits_only));
			BN_HIP(hipStreamSynchronize(ctx->stream)); // (the tables are pageable host memory that goes out of scope; the fold_left launches may regrow the scratch)
		}
	}
	for (uint32_t c : wide) {
		const int rc = fold_left_dispatch(ctx, cols[c].d_evals, cols[c].tower_level, d_vec, (uint64_t)1 << q, d_outs[c], (uint64_t)1 << (cols[c].n_vars - q));
		if (rc) return rc;
	}
	// (a call that failed on the way counts nowhere)
	if (!order.empty()) ctx->pe_launches += 2; // k_pe_zero + k_partial_eval
	ctx->pe_cols_kernel += order.size();
	ctx->pe_cols_fallback += wide.size();
	ctx->pe_max_share = max_share;
	if (routed)
		ctx->pe_routed++;
	else
		ctx->pe_calls++;
	return BN_OK;
}

} // namespace bnabi

extern "C" {

int bn_partial_eval_high_batch(bn_ctx *ctx, const void *cols_, uint32_t n_cols, const void *d_tensor_query, uint32_t query_vars, void *const *d_outs)
{
	const bn_pe_column *cols = (const bn_pe_column *)cols_;
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n_cols == 0) return BN_OK;
	BN_REQUIRE(cols && d_tensor_query && d_outs, "null argument");
	BN_REQUIRE(n_cols <= (1u << 20), "too many columns for one call");
	BN_REQUIRE(query_vars <= BN_PE_MAX_VARS, "partial eval: query_vars out of range");
	BN_REQUIRE(aligned16(d_tensor_query), "partial eval: pointers must be 16-byte aligned");
	for (uint32_t c = 0; c < n_cols; c++) {
		BN_REQUIRE(cols[c].d_evals && d_outs[c], "partial eval: null pointer");
		BN_REQUIRE(cols[c].tower_level <= 7, "invalid evals: tower_level > 7");
		BN_REQUIRE(valid_tower_level(cols[c].tower_level), "unsupported value of tower_level");
		BN_REQUIRE(cols[c].n_vars <= BN_PE_MAX_VARS && cols[c].n_vars + cols[c].tower_level >= 7, "partial eval: a column is at least one 128-bit element, at most 2^40 values");
		BN_REQUIRE(query_vars <= cols[c].n_vars, "query larger than evals");
		BN_REQUIRE(aligned16(cols[c].d_evals, d_outs[c]), "partial eval: pointers must be 16-byte aligned");
		BN_REQUIRE(!ranges_overlap(cols[c].d_evals, column_elems(cols[c].n_vars, cols[c].tower_level), d_outs[c], (uint64_t)1 << (cols[c].n_vars - query_vars)),
		           "partial eval: an output overlaps its column");
	}
	return partial_eval_run(ctx, cols, n_cols, d_tensor_query, query_vars, d_outs, false);
}

int bn_partial_eval_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_PE_CALLS] = ctx->pe_calls;
	counters[BN_PE_LAUNCHES] = ctx->pe_launches;
	counters[BN_PE_COLS_KERNEL] = ctx->pe_cols_kernel;
	counters[BN_PE_COLS_FALLBACK] = ctx->pe_cols_fallback;
	counters[BN_PE_MAX_SHARE] = ctx->pe_max_share;
	counters[BN_PE_FOLD_LEFT_ROUTED] = ctx->pe_routed;
	return BN_OK;
}

} // extern "C"
