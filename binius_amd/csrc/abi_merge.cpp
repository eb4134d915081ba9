// binius_amd/csrc/abi_merge.cpp -- bn_merge_multilins: merge_multilins (crates/core/src/piop/prove.rs:78-118, P = F) for multilinears
// resident on the device.  Argument validation and the plan of the launch; the kernel is in kernels_merge.hip.
//
// The plan: one job per multilinear, last multilinear first (it lands at offset 0), tiled from 2 t variables, small below; one more
// job for the zero tail of every repeat.  Jobs are packed into launches of at most kMergeLaunchJobs jobs and kMergeLaunchUnits
// workgroups: a job that does not fit continues in the next launch (merge_job::first).  One upload carries the tables of all launches.
#include <algorithm>

#include "abi_common.hpp"

static uint32_t merge_tile_log2()
{
	// (a measurement build compares t = 5 and t = 6 in one process: read per call)
	const char *e = bn::settled_knob("BN_MERGE_T");
	return e && e[0] >= '5' && e[0] <= '6' && !e[1] ? (uint32_t)(e[0] - '0') : (uint32_t)BN_MERGE_TILE_LOG2;
}

extern "C" {

int bn_merge_multilins(bn_ctx *ctx, uint32_t n, const uint32_t *n_vars, const void *const *d_multilins, void *d_message, uint32_t total_vars, uint32_t log_repeats)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_REQUIRE(d_message && (n == 0 || (n_vars && d_multilins)), "merge_multilins: null argument");
	BN_REQUIRE(aligned16(d_message), "merge_multilins: pointers must be 16-byte aligned");
	BN_REQUIRE(total_vars < 48 && log_repeats < 48 && total_vars + log_repeats < 48, "merge_multilins: total_vars + log_repeats out of range (< 48)");
	const uint64_t cap = (uint64_t)1 << total_vars, dst_elems = cap << log_repeats;
	uint64_t sum = 0;
	for (uint32_t i = 0; i < n; i++) {
		BN_REQUIRE(d_multilins[i], "merge_multilins: null multilinear");
		BN_REQUIRE(aligned16(d_multilins[i]), "merge_multilins: pointers must be 16-byte aligned");
		BN_REQUIRE(n_vars[i] < 48, "merge_multilins: n_vars out of range (< 48)");
		BN_REQUIRE(i == 0 || n_vars[i] >= n_vars[i - 1], "CommittedsNotSorted: the multilinears must be ascending by number of variables");
		sum += (uint64_t)1 << n_vars[i]; // (at most 2^47 past a value that passed the check below)
		BN_REQUIRE(sum <= cap, "merge_multilins: the multilinears hold more than 2^total_vars elements");
	}
	for (uint32_t i = 0; i < n; i++)
		BN_REQUIRE(!ranges_overlap(d_multilins[i], (uint64_t)1 << n_vars[i], d_message, dst_elems), "merge_multilins: a multilinear overlaps the message");
	BN_FLUSH(ctx);

	// ---- the jobs, in message order, cut into launches
	const uint32_t t = merge_tile_log2();
	struct launch {
		uint32_t first_job, n_jobs, units;
	};
	std::vector<bn::merge_job> table;
	std::vector<launch> launches{launch{0, 0, 0}};
	auto add = [&](bn::merge_job jb, uint64_t units) {
		for (uint64_t done = 0; done < units;) {
			if (launches.back().n_jobs == bn::kMergeLaunchJobs || launches.back().units == bn::kMergeLaunchUnits)
				launches.push_back(launch{(uint32_t)table.size(), 0, 0});
			launch &l = launches.back();
			const uint64_t take = std::min<uint64_t>(units - done, bn::kMergeLaunchUnits - l.units);
			jb.first = done;
			jb.start = l.units;
			table.push_back(jb);
			l.n_jobs++;
			l.units += (uint32_t)take;
			done += take;
		}
	};
	uint64_t off = 0, n_tiled = 0, n_small = 0;
	for (uint32_t i = n; i-- > 0;) {
		const uint32_t L = n_vars[i];
		const bool tiled = L >= 2 * t;
		add(bn::merge_job{d_multilins[i], off, 0, 0, L, tiled ? bn::kMergeTiled : bn::kMergeSmall, 0, 0}, tiled ? (uint64_t)1 << (L - 2 * t) : 1);
		(tiled ? n_tiled : n_small)++;
		off += (uint64_t)1 << L;
	}
	uint64_t n_jobs = n;
	if (off < cap) {
		add(bn::merge_job{nullptr, off, 0, cap - off, 0, bn::kMergeZero, 0, 0}, (cap - off + bn::kMergeZeroChunk - 1) / bn::kMergeZeroChunk);
		n_jobs++;
	}

	call_upload up(ctx);
	const auto s_jobs = up.reserve<bn::merge_job>(table.size());
	if (const int rc = up.alloc()) return rc;
	std::copy(table.begin(), table.end(), up.host(s_jobs));
	BN_HIP(up.send());
	uint64_t n_launches = 0;
	for (const launch &l : launches) {
		if (l.n_jobs == 0) continue;
		BN_HIP(bn::launch_merge_multilins(ctx->stream, t, up.dev(s_jobs) + l.first_job, l.n_jobs, d_message, total_vars, log_repeats, l.units));
		n_launches++;
	}
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the table is pageable host memory that goes out of scope; the message is complete on return)
	ctx->mg_calls++;
	ctx->mg_launches += n_launches;
	ctx->mg_jobs += n_jobs;
	ctx->mg_jobs_tiled += n_tiled;
	ctx->mg_jobs_small += n_small;
	return BN_OK;
}

int bn_merge_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_MERGE_CALLS] = ctx->mg_calls;
	counters[BN_MERGE_LAUNCHES] = ctx->mg_launches;
	counters[BN_MERGE_JOBS] = ctx->mg_jobs;
	counters[BN_MERGE_JOBS_TILED] = ctx->mg_jobs_tiled;
	counters[BN_MERGE_JOBS_SMALL] = ctx->mg_jobs_small;
	return BN_OK;
}

} // extern "C"
