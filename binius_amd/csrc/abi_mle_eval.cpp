// binius_amd/csrc/abi_mle_eval.cpp -- bn_mle_evaluate_batch: a batch of columns evaluated at their whole claim points, the first step of
// every EvalcheckProver::prove call (core/src/protocols/evalcheck/prove.rs:191-275, make_new_eval_claim :812-879; evaluate_partial_high
// followed by evaluate, math/src/multilinear_extension.rs).  Argument validation and the plan of the launch; the kernel is in
// kernels_mle_eval.hip.
//
// The plan: the jobs are sorted by class (point, tower level) and cut into groups of up to G jobs of one class, G <= kMeGroupJobs and
// G * 2^lo_vars <= kMeAccs (the accumulators of a group live in LDS).  A unit (one workgroup) is a chunk of 2^log_ch rows of one group.
// The epilogue (2^lo_vars full products per job) is paid once per unit and job, so the chunk starts at ALL rows of the column and is
// halved only while the launch would not fill the device; it never gets smaller than 2 KiB of column.  At the chunk size found, the
// largest G that still fills the device is taken: it costs no epilogue and shares the staged rows of `hi`.  One upload carries the
// zeroed result slots, the group table and the job table; the second launch publishes the slots through pinned memory.
#include <algorithm>

#include "abi_common.hpp"

namespace {

// the smallest chunk (log2 rows) of a class: a 64-bit word of a bit column is not split between units, 2 KiB of column per unit
uint32_t me_min_log_ch(uint32_t level, uint32_t b, uint32_t q)
{
	const uint32_t word = (level == 0 && b < 6) ? 6 - b : 0;
	const uint32_t row = b + level; // log2 of the bits of a row
	return std::min(std::max(word, row >= 14 ? 0 : 14 - row), q);
}

int me_rets_alloc(bn_ctx *ctx)
{
	if (ctx->h_me_rets) return BN_OK;
	if (hipHostMalloc((void **)&ctx->h_me_rets, sizeof(f128) * BN_ME_MAX_JOBS, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
		(void)hipGetLastError();
		ctx->h_me_rets = nullptr;
		return bn::fail(BN_ERR_ALLOC, "allocation error: pinned result area of bn_mle_evaluate_batch");
	}
	std::memset(ctx->h_me_rets, 0, sizeof(f128) * BN_ME_MAX_JOBS);
	BN_HIP(hipHostGetDevicePointer((void **)&ctx->d_me_rets, ctx->h_me_rets, 0));
	return BN_OK;
}

} // namespace

extern "C" {

int bn_mle_evaluate_batch(bn_ctx *ctx, const void *jobs_, uint32_t n_jobs, const void *points_, uint32_t n_points, bn_f128 *h_out)
{
	const bn_me_job *jobs = (const bn_me_job *)jobs_;
	const bn_me_point *points = (const bn_me_point *)points_;
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n_jobs == 0) return BN_OK;
	BN_REQUIRE(jobs && points && h_out, "null argument");
	BN_REQUIRE(n_jobs <= BN_ME_MAX_JOBS, "mle evaluate: too many jobs for one call");
	for (uint32_t p = 0; p < n_points; p++) {
		BN_REQUIRE(points[p].d_lo && points[p].d_hi, "mle evaluate: null table");
		BN_REQUIRE(aligned16(points[p].d_lo, points[p].d_hi), "mle evaluate: pointers must be 16-byte aligned");
		BN_REQUIRE(points[p].lo_vars <= BN_ME_MAX_LO_VARS, "mle evaluate: lo_vars out of range");
		BN_REQUIRE(points[p].hi_vars <= BN_PE_MAX_VARS, "mle evaluate: hi_vars out of range");
	}
	for (uint32_t j = 0; j < n_jobs; j++) {
		const bn_me_job &jb = jobs[j];
		BN_REQUIRE(jb.d_evals, "mle evaluate: null pointer");
		BN_REQUIRE(aligned16(jb.d_evals), "mle evaluate: pointers must be 16-byte aligned");
		BN_REQUIRE(jb.reserved == 0, "mle evaluate: reserved must be 0");
		BN_REQUIRE(jb.tower_level <= 7, "invalid evals: tower_level > 7");
		BN_REQUIRE(valid_tower_level(jb.tower_level), "unsupported value of tower_level");
		BN_REQUIRE(jb.point < n_points, "mle evaluate: a job names a point outside the point table");
		BN_REQUIRE(jb.n_vars <= BN_PE_MAX_VARS && jb.n_vars + jb.tower_level >= 7, "mle evaluate: a column is at least one 128-bit element, at most 2^40 values");
		BN_REQUIRE(points[jb.point].lo_vars + points[jb.point].hi_vars == jb.n_vars, "mle evaluate: lo_vars + hi_vars must equal n_vars");
	}

	// ---- the jobs sorted by class
	std::vector<uint32_t> order(n_jobs);
	for (uint32_t j = 0; j < n_jobs; j++) order[j] = j;
	auto key = [&](uint32_t j) { return ((uint64_t)jobs[j].point << 8) | jobs[j].tower_level; };
	std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return key(x) < key(y); });
	std::vector<bn::me_group> groups;
	uint64_t units = 0, max_share = 0;
	// units of the launch with chunks `shrink` halvings below all rows and groups of up to G jobs (fills `groups`)
	auto plan = [&](uint32_t shrink, uint32_t G) {
		groups.clear();
		units = 0;
		max_share = 0;
		for (uint32_t at = 0; at < n_jobs;) {
			const bn_me_job &j0 = jobs[order[at]];
			const bn_me_point &pt = points[j0.point];
			const uint32_t b = pt.lo_vars, q = pt.hi_vars;
			const uint32_t g_max = std::min(G, std::min(bn::kMeGroupJobs, bn::kMeAccs >> b));
			uint32_t end = at;
			while (end < n_jobs && end - at < g_max && key(order[end]) == key(order[at])) end++;
			const uint32_t floor_ch = me_min_log_ch(j0.tower_level, b, q);
			const uint32_t log_ch = q - std::min(shrink, q - floor_ch);
			const uint64_t n_chunks = (uint64_t)1 << (q - log_ch);
			groups.push_back(bn::me_group{pt.d_lo, pt.d_hi, at, end - at, j0.tower_level, b, log_ch, (uint32_t)std::min<uint64_t>(units, 0xFFFFFFFFu)});
			units += n_chunks;
			max_share = std::max(max_share, n_chunks);
			at = end;
		}
	};
	const uint64_t want = (uint64_t)ctx->n_cu * 4;
	uint32_t shrink = 0, max_shrink = 0; // (beyond every class's smallest chunk nothing changes any more)
	for (uint32_t j = 0; j < n_jobs; j++) {
		const bn_me_point &pt = points[jobs[j].point];
		max_shrink = std::max(max_shrink, pt.hi_vars - me_min_log_ch(jobs[j].tower_level, pt.lo_vars, pt.hi_vars));
	}
	for (;; shrink++) {
		plan(shrink, 1);
		if (units >= want || shrink >= max_shrink) break;
	}
	for (uint32_t G = bn::kMeGroupJobs; G >= 1; G /= 2) {
		plan(shrink, G);
		if (units >= want || G == 1) break;
	}
	BN_REQUIRE(units < (1ull << 31), "mle evaluate: batch too large for one call");

	if (const int rc = me_rets_alloc(ctx)) return rc;
	// ---- one upload: [slots (zero)][groups][jobs]
	call_upload up(ctx);
	const auto s_slots = up.reserve<f128>(n_jobs);
	const auto s_groups = up.reserve<bn::me_group>(groups.size());
	const auto s_jobs = up.reserve<bn::me_job>(n_jobs);
	if (const int rc = up.alloc()) return rc;
	std::copy(groups.begin(), groups.end(), up.host(s_groups));
	bn::me_job *table = up.host(s_jobs);
	bool bits_only = true;
	for (uint32_t i = 0; i < n_jobs; i++) {
		table[i] = bn::me_job{(const uint64_t *)jobs[order[i]].d_evals, (uint64_t *)(up.dev(s_slots) + order[i])};
		bits_only = bits_only && jobs[order[i]].tower_level == 0;
	}
	BN_HIP(up.send());
	BN_HIP(bn::launch_mle_eval(ctx->stream, up.dev(s_groups), (uint32_t)groups.size(), up.dev(s_jobs), (uint32_t)units, bits_only));
	const uint64_t seq = ++ctx->mail_seq;
	BN_HIP(bn::launch_me_publish(ctx->stream, up.dev(s_slots), n_jobs, ctx->d_me_rets, ctx->d_mail, seq));
	// (the sequence word is written behind the upload in stream order: the pageable mirror may go out of scope)
	if (const int rc = mail_wait(ctx, seq)) return rc;
	for (uint32_t j = 0; j < n_jobs; j++) {
		h_out[j].lo = __atomic_load_n(&ctx->h_me_rets[j].lo, __ATOMIC_RELAXED);
		h_out[j].hi = __atomic_load_n(&ctx->h_me_rets[j].hi, __ATOMIC_RELAXED);
	}
	ctx->me_calls++;
	ctx->me_launches += 2; // k_mle_eval + k_me_publish
	ctx->me_jobs += n_jobs;
	ctx->me_max_share = max_share;
	return BN_OK;
}

int bn_mle_evaluate_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_ME_CALLS] = ctx->me_calls;
	counters[BN_ME_LAUNCHES] = ctx->me_launches;
	counters[BN_ME_JOBS] = ctx->me_jobs;
	counters[BN_ME_MAX_SHARE] = ctx->me_max_share;
	return BN_OK;
}

} // extern "C"
