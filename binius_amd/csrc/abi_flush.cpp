// binius_amd/csrc/abi_flush.cpp -- bn_flush_witness_batch: the masked flush witnesses of a batch of channel flushes
// (make_masked_flush_witnesses, core/src/constraint_system/prove.rs:671-881; the selectors' prefix: count_zero_suffixes, :883-902).
// Argument validation and the plan of the launches; the kernels are in kernels_flush.hip.
//
// The plan: one job per flush, ceil(2^n_vars / 2048) units each, ONE launch of the main kernel for the call, after ONE launch of the
// selector pre-pass when the call has a selector at all.  The columns of a flush are dealt out to passes of at most 256 nibble
// tables (64 KiB of LDS): 2^level / 4 tables per column, none for a bit column or a coefficient ONE.  One upload carries the job
// table, the column descriptors, the selector pointers, the pre-pass's table and the zeroed prefix words; one read-back after the
// main kernel returns the prefix words, from which the host forms prefix_lens_out.
#include <algorithm>

#include "abi_common.hpp"

namespace {

struct span {
	uintptr_t b, e;
	bool operator<(const span &o) const { return b < o.b; }
};

// does any output overlap an input of the call (of its own flush or of another one), or another output?
bool outputs_clash(std::vector<span> &ins, std::vector<span> &outs)
{
	std::sort(ins.begin(), ins.end());
	std::sort(outs.begin(), outs.end());
	for (size_t i = 1; i < outs.size(); i++)
		if (outs[i].b < outs[i - 1].e) return true;
	std::vector<uintptr_t> reach(ins.size()); // the furthest end among the inputs that begin no later than input i
	for (size_t i = 0; i < ins.size(); i++) reach[i] = std::max(ins[i].e, i ? reach[i - 1] : 0);
	for (const span &o : outs) {
		const size_t k = std::lower_bound(ins.begin(), ins.end(), span{o.e, 0}) - ins.begin(); // inputs [0, k) begin before the output ends
		if (k && reach[k - 1] > o.b) return true;
	}
	return false;
}

} // namespace

extern "C" {

int bn_flush_witness_batch(bn_ctx *ctx, uint32_t n_flushes, const uint32_t *n_vars, const uint32_t *n_selectors, const void *const *d_selectors,
                           const uint32_t *n_columns, const void *const *d_columns, const uint32_t *tower_levels, const bn_f128 *coeffs,
                           const bn_f128 *const_terms, void *const *d_outs, uint64_t *prefix_lens_out)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n_flushes == 0) return BN_OK;
	BN_REQUIRE(n_vars && n_selectors && n_columns && const_terms && d_outs && prefix_lens_out, "null argument");
	BN_REQUIRE(n_flushes <= (1u << 16), "too many flushes for one call");
	size_t n_cols = 0, n_sels = 0;
	uint64_t units = 0, sel_wgs = 0;
	std::vector<span> ins, outs;
	for (uint32_t f = 0; f < n_flushes; f++) {
		BN_REQUIRE(n_vars[f] <= BN_FLUSH_MAX_VARS, "flush witness: n_vars out of range (0 .. 28)");
		BN_REQUIRE(n_selectors[f] <= BN_FLUSH_MAX_SELECTORS, "flush witness: more than 8 selectors");
		BN_REQUIRE(n_columns[f] >= 1, "flush witness: EmptyFlushOracles (a flush without columns)");
		BN_REQUIRE(n_columns[f] <= BN_FLUSH_MAX_COLUMNS, "flush witness: more than 64 columns");
		BN_REQUIRE(d_columns && tower_levels && coeffs, "null argument");
		BN_REQUIRE(n_selectors[f] == 0 || d_selectors, "null argument");
		const uint64_t rows = (uint64_t)1 << n_vars[f];
		BN_REQUIRE(d_outs[f], "flush witness: null output");
		BN_REQUIRE(aligned16(d_outs[f]), "flush witness: pointers must be 16-byte aligned");
		for (uint32_t s = 0; s < n_selectors[f]; s++) {
			const void *sel = d_selectors[n_sels + s];
			BN_REQUIRE(sel, "flush witness: null selector");
			BN_REQUIRE(aligned16(sel), "flush witness: pointers must be 16-byte aligned");
			ins.push_back(span{(uintptr_t)sel, (uintptr_t)sel + 16 * column_elems(n_vars[f], 0)});
			sel_wgs += (column_elems(n_vars[f], 0) + bn::kFlushSelChunk - 1) / bn::kFlushSelChunk;
		}
		for (uint32_t j = 0; j < n_columns[f]; j++) {
			const void *col = d_columns[n_cols + j];
			const uint32_t level = tower_levels[n_cols + j];
			BN_REQUIRE(valid_tower_level(level), "flush witness: tower level must be 0 or 3 .. 7");
			BN_REQUIRE(col, "flush witness: null column");
			BN_REQUIRE(aligned16(col), "flush witness: pointers must be 16-byte aligned");
			ins.push_back(span{(uintptr_t)col, (uintptr_t)col + 16 * column_elems(n_vars[f], level)});
		}
		outs.push_back(span{(uintptr_t)d_outs[f], (uintptr_t)d_outs[f] + 16 * rows});
		n_cols += n_columns[f];
		n_sels += n_selectors[f];
		units += (rows + bn::kFlushUnitRows - 1) / bn::kFlushUnitRows;
		BN_REQUIRE(units < (1ull << 31) && sel_wgs < (1ull << 31), "flush witness: batch too large for one call");
	}
	BN_REQUIRE(!outputs_clash(ins, outs), "flush witness: an output overlaps an input or another output of the call");

	// ---- one upload: [jobs][column descriptors][selector pointers][pre-pass table][prefix words]
	call_upload up(ctx);
	const auto s_jobs = up.reserve<bn::flush_job>(n_flushes);
	const auto s_cols = up.reserve<bn::flush_col>(n_cols);
	const auto s_ptrs = up.reserve<const uint32_t *>(n_sels);
	const auto s_sels = up.reserve<bn::flush_sel>(n_sels);
	const auto s_pref = up.reserve<uint64_t>(n_sels); // (uploaded as zeros; the pre-pass raises them)
	if (const int rc = up.alloc()) return rc;
	bn::flush_job *jobs = up.host(s_jobs);
	bn::flush_col *cols = up.host(s_cols);
	bn::flush_sel *sels = up.host(s_sels);
	if (n_sels) memcpy(up.host(s_ptrs), d_selectors, n_sels * sizeof(void *));
	size_t at_col = 0, at_sel = 0;
	uint32_t at_unit = 0, at_wg = 0, multipass = 0;
	for (uint32_t f = 0; f < n_flushes; f++) {
		bn::flush_job &jb = jobs[f];
		jb.cols = up.dev(s_cols) + at_col;
		jb.sels = up.dev(s_ptrs) + at_sel;
		jb.sel_prefix = up.dev(s_pref) + at_sel;
		jb.out = (uint4 *)d_outs[f];
		jb.const_term = to_f(&const_terms[f]);
		jb.rows = (uint64_t)1 << n_vars[f];
		jb.n_cols = n_columns[f];
		jb.n_sels = n_selectors[f];
		jb.start = at_unit;
		uint32_t pass = 0, used = 0;
		jb.pass_first[0] = 0;
		for (uint32_t j = 0; j < n_columns[f]; j++) {
			bn::flush_col &c = cols[at_col + j];
			c.ptr = d_columns[at_col + j];
			c.coeff = to_f(&coeffs[at_col + j]);
			c.level = tower_levels[at_col + j];
			const bool plain = c.level == 0 || c.coeff == bn::f128_one();
			const uint32_t tables = plain ? 0 : (1u << c.level) / 4;
			if (used + tables > bn::kFlushPassTables) {
				jb.pass_first[++pass] = j;
				used = 0;
			}
			c.table = plain ? bn::kFlushNoTable : used;
			used += tables;
		}
		jb.n_passes = pass + 1;
		jb.pass_first[jb.n_passes] = n_columns[f];
		if (jb.n_passes > 1) multipass++;
		for (uint32_t s = 0; s < n_selectors[f]; s++) {
			bn::flush_sel &sl = sels[at_sel + s];
			sl.col = (const uint4 *)d_selectors[at_sel + s];
			sl.prefix = up.dev(s_pref) + at_sel + s;
			sl.elems = column_elems(n_vars[f], 0);
			sl.start = at_wg;
			at_wg += (uint32_t)((sl.elems + bn::kFlushSelChunk - 1) / bn::kFlushSelChunk);
		}
		at_col += n_columns[f];
		at_sel += n_selectors[f];
		at_unit += (uint32_t)((jb.rows + bn::kFlushUnitRows - 1) / bn::kFlushUnitRows);
	}
	BN_HIP(up.send());
	BN_HIP(bn::launch_flush_prefix(ctx->stream, up.dev(s_sels), (uint32_t)n_sels, at_wg));
	BN_HIP(bn::launch_flush_witness(ctx->stream, up.dev(s_jobs), n_flushes, at_unit));
	std::vector<uint64_t> pref(n_sels);
	if (n_sels) BN_HIP(hipMemcpyAsync(pref.data(), up.dev(s_pref), n_sels * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	ctx->flush_calls++;
	ctx->flush_launches += n_sels ? 2 : 1;
	ctx->flush_served += n_flushes;
	ctx->flush_multipass += multipass;
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the witnesses are complete and the prefixes on the host on return)
	at_sel = 0;
	for (uint32_t f = 0; f < n_flushes; f++) {
		uint64_t len = (uint64_t)1 << n_vars[f];
		for (uint32_t s = 0; s < n_selectors[f]; s++) len = std::min(len, pref[at_sel + s]);
		prefix_lens_out[f] = len;
		at_sel += n_selectors[f];
	}
	return BN_OK;
}

int bn_flush_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_FLUSH_CALLS] = ctx->flush_calls;
	counters[BN_FLUSH_LAUNCHES] = ctx->flush_launches;
	counters[BN_FLUSH_SERVED] = ctx->flush_served;
	counters[BN_FLUSH_MULTIPASS] = ctx->flush_multipass;
	return BN_OK;
}

} // extern "C"
