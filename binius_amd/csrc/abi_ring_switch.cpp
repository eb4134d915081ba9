// binius_amd/csrc/abi_ring_switch.cpp -- bn_ring_switch_eq_ind_batch: every ring-switch equality indicator of a call
// (RingSwitchEqInd::multilinear_extension, core/src/ring_switch/eq_ind.rs:81-147; one per claim of ring_switch::prove,
// core/src/ring_switch/prove.rs:116-124).  Argument validation and the plan of the launch; the kernel is in kernels_ring_switch.hip.
//
// The plan: the jobs are sorted by (query, n_vars, kappa) and cut into runs of up to kRsRunJobs jobs of one query; a unit (one workgroup) is
// a run and `span` consecutive tiles of kRsTile elements, span the largest of 1, 2, 4, 8 that still leaves four units per CU (the
// tables of a run are built once per unit).  One upload carries the coefficients, the run table and the job table.
#include <algorithm>

#include "abi_common.hpp"

extern "C" {

int bn_ring_switch_eq_ind_batch(bn_ctx *ctx, const void *jobs_, uint32_t n_jobs, const bn_f128 *h_row_batch_coeffs, uint32_t n_coeffs, void *const *d_outs)
{
	const bn_rs_job *jobs = (const bn_rs_job *)jobs_;
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n_jobs == 0) return BN_OK;
	BN_REQUIRE(jobs && h_row_batch_coeffs && d_outs, "null argument");
	BN_REQUIRE(n_jobs <= (1u << 20), "too many jobs for one call");
	BN_REQUIRE(is_pow2(n_coeffs), "ring switch: the number of row-batch coefficients must be a power of two");
	struct range {
		uintptr_t lo, hi;
		bool out;
	};
	std::vector<range> ranges;
	ranges.reserve(2 * (size_t)n_jobs);
	for (uint32_t j = 0; j < n_jobs; j++) {
		const bn_rs_job &jb = jobs[j];
		BN_REQUIRE(jb.d_query && d_outs[j], "ring switch: null pointer");
		BN_REQUIRE(aligned16(jb.d_query, d_outs[j]), "ring switch: pointers must be 16-byte aligned");
		BN_REQUIRE(jb.n_vars <= BN_PE_MAX_VARS, "ring switch: n_vars out of range");
		BN_REQUIRE(jb.kappa <= 7 && valid_tower_level(7 - jb.kappa), "ring switch: kappa must be one of 0, 1, 2, 3, 4, 7");
		BN_REQUIRE(((uint64_t)1 << jb.kappa) <= n_coeffs, "ring switch: fewer row-batch coefficients than the extension degree");
		const uintptr_t bytes = (uintptr_t)16 << jb.n_vars;
		ranges.push_back(range{(uintptr_t)jb.d_query, (uintptr_t)jb.d_query + bytes, false});
		ranges.push_back(range{(uintptr_t)d_outs[j], (uintptr_t)d_outs[j] + bytes, true});
	}
	// an output overlaps nothing else of the call (queries may coincide: they are only read)
	std::sort(ranges.begin(), ranges.end(), [](const range &a, const range &b) { return a.lo < b.lo; });
	uintptr_t end_any = 0, end_out = 0;
	for (const range &r : ranges) {
		BN_REQUIRE(r.lo >= (r.out ? end_any : end_out), "ring switch: an output overlaps a query or another output");
		end_any = std::max(end_any, r.hi);
		if (r.out) end_out = std::max(end_out, r.hi);
	}

	// ---- the runs: jobs sorted by (query, n_vars, kappa), up to kRsRunJobs of one query each
	std::vector<uint32_t> order(n_jobs);
	for (uint32_t j = 0; j < n_jobs; j++) order[j] = j;
	auto same = [&](uint32_t x, uint32_t y) { return jobs[x].d_query == jobs[y].d_query && jobs[x].n_vars == jobs[y].n_vars; };
	std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
		if (jobs[x].d_query != jobs[y].d_query) return (uintptr_t)jobs[x].d_query < (uintptr_t)jobs[y].d_query;
		return jobs[x].n_vars != jobs[y].n_vars ? jobs[x].n_vars < jobs[y].n_vars : jobs[x].kappa < jobs[y].kappa; // (one kappa after the other: its bit images are built once)
	});
	std::vector<bn::rs_run> runs;
	uint64_t n_queries = 0, tiles_total = 0;
	for (uint32_t at = 0; at < n_jobs;) {
		uint32_t end = at;
		while (end < n_jobs && end - at < bn::kRsRunJobs && same(order[end], order[at])) end++;
		if (at == 0 || jobs[order[at]].d_query != jobs[order[at - 1]].d_query) n_queries++;
		const uint64_t len = (uint64_t)1 << jobs[order[at]].n_vars;
		runs.push_back(bn::rs_run{jobs[order[at]].d_query, len, at, end - at, 0, 0});
		tiles_total += (len + bn::kRsTile - 1) / bn::kRsTile;
		BN_REQUIRE(tiles_total < (1ull << 31), "ring switch: batch too large for one call");
		at = end;
	}
	auto units_at = [&](uint32_t span) {
		uint64_t u = 0;
		for (const bn::rs_run &r : runs) u += ((r.len + bn::kRsTile - 1) / bn::kRsTile + span - 1) / span;
		return u;
	};
	uint32_t span = 1;
	while (span < 8 && units_at(2 * span) >= (uint64_t)ctx->n_cu * 4) span *= 2;
	uint32_t at_unit = 0;
	for (bn::rs_run &r : runs) {
		r.start = at_unit;
		at_unit += (uint32_t)(((r.len + bn::kRsTile - 1) / bn::kRsTile + span - 1) / span);
	}

	// ---- one upload: [coefficients][runs][jobs]
	const uint32_t n_staged = std::min<uint32_t>(n_coeffs, 128);
	call_upload up(ctx);
	const auto s_coeffs = up.reserve<bn_f128>(n_staged);
	const auto s_runs = up.reserve<bn::rs_run>(runs.size());
	const auto s_jobs = up.reserve<bn::rs_job>(n_jobs);
	if (const int rc = up.alloc()) return rc;
	std::copy(h_row_batch_coeffs, h_row_batch_coeffs + n_staged, up.host(s_coeffs));
	std::copy(runs.begin(), runs.end(), up.host(s_runs));
	bn::rs_job *table = up.host(s_jobs);
	for (uint32_t i = 0; i < n_jobs; i++) {
		const bn_rs_job &jb = jobs[order[i]];
		table[i].out = (uint4 *)d_outs[order[i]];
		table[i].mixing = f128{jb.mixing_coeff.lo, jb.mixing_coeff.hi};
		table[i].kappa = jb.kappa;
	}
	BN_HIP(up.send());
	BN_HIP(bn::launch_ring_switch_eq_ind(ctx->stream, up.dev(s_runs), (uint32_t)runs.size(), up.dev(s_jobs), up.dev(s_coeffs), n_staged, span, at_unit));
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the tables are pageable host memory that goes out of scope; the outputs are complete on return)
	ctx->rs_calls++;
	ctx->rs_launches++;
	ctx->rs_jobs += n_jobs;
	ctx->rs_queries += n_queries;
	return BN_OK;
}

int bn_ring_switch_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_RS_CALLS] = ctx->rs_calls;
	counters[BN_RS_LAUNCHES] = ctx->rs_launches;
	counters[BN_RS_JOBS] = ctx->rs_jobs;
	counters[BN_RS_QUERIES] = ctx->rs_queries;
	return BN_OK;
}

} // extern "C"
