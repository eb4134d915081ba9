// binius_amd/csrc/abi_partial_eval_lincomb.cpp -- bn_partial_eval_high_lincomb_batch: the projection of bn_partial_eval_high_batch for
// inner columns that are linear combinations of columns and are never materialised (try_build_partial_eval, core/src/protocols/
// evalcheck/subclaims.rs:305-346).  Argument validation and the plan of the launches; the kernels are in
// kernels_partial_eval_lincomb.hip.
//
// The plan: inside a job the terms with a non-zero coefficient are sorted by (tower level, coefficient); a run of equal keys is a
// class -- one row loop over the XOR of its columns.  A job with at most 1024 outputs is cut into units (workgroups) of 2^log_ch
// reduction indices; log_ch starts at 8 KiB per unit of the job's widest column and is halved (twice at most) while the call would
// not fill the device, as bn_partial_eval_high_batch plans a group of one column.  One upload carries the job, class and column-pointer
// tables.  Jobs with more outputs share one launch of the one-thread-per-output form.
#include <algorithm>

#include "abi_common.hpp"

namespace {

struct pel_range {
	uintptr_t begin, end;
	bool output;
};

uint32_t pel_log_ch(uint32_t max_level, bool has_bits, uint32_t b, uint32_t q, uint32_t shrink)
{
	const uint32_t lo = (has_bits && b < 6) ? 6 - b : 0; // a 64-bit word of a bit column is not split between units
	const uint32_t row = b + max_level;                  // log2 of the bits of a row of the widest column
	uint32_t l = row >= 16 ? 0 : 16 - row;               // 8 KiB of that column per unit
	l = std::min(l, bn::kPeLogVecChunk);
	l = l > shrink ? l - shrink : 0;
	l = std::max(l, lo);
	return std::min(l, q);
}

} // namespace

extern "C" {

int bn_partial_eval_high_lincomb_batch(bn_ctx *ctx, const void *jobs_, uint32_t n_jobs, const void *terms_, uint32_t n_terms_total, const void *d_tensor_query,
                                       uint32_t query_vars, void *const *d_outs)
{
	const bn_pel_job *jobs = (const bn_pel_job *)jobs_;
	const bn_pel_term *terms = (const bn_pel_term *)terms_;
	const uint32_t q = query_vars;
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n_jobs == 0) return BN_OK;
	BN_REQUIRE(jobs && d_tensor_query && d_outs && (terms || n_terms_total == 0), "null argument");
	BN_REQUIRE(n_jobs <= (1u << 20), "too many jobs for one call");
	BN_REQUIRE(q <= BN_PE_MAX_VARS, "partial eval: query_vars out of range");
	BN_REQUIRE(aligned16(d_tensor_query), "partial eval: pointers must be 16-byte aligned");
	for (uint32_t t = 0; t < n_terms_total; t++) {
		BN_REQUIRE(terms[t].d_evals, "partial eval: null pointer");
		BN_REQUIRE(aligned16(terms[t].d_evals), "partial eval: pointers must be 16-byte aligned");
		BN_REQUIRE(terms[t].tower_level <= 7, "invalid evals: tower_level > 7");
		BN_REQUIRE(valid_tower_level(terms[t].tower_level), "unsupported value of tower_level");
		BN_REQUIRE(terms[t].reserved == 0, "partial eval: reserved must be 0");
	}
	std::vector<pel_range> ranges;
	ranges.push_back(pel_range{(uintptr_t)d_tensor_query, (uintptr_t)d_tensor_query + ((uintptr_t)16 << q), false});
	for (uint32_t j = 0; j < n_jobs; j++) {
		const bn_pel_job &jb = jobs[j];
		BN_REQUIRE(d_outs[j], "partial eval: null pointer");
		BN_REQUIRE(aligned16(d_outs[j]), "partial eval: pointers must be 16-byte aligned");
		BN_REQUIRE(jb.reserved == 0, "partial eval: reserved must be 0");
		BN_REQUIRE(jb.n_vars <= BN_PE_MAX_VARS, "partial eval: a column has at most 2^40 values");
		BN_REQUIRE(q <= jb.n_vars, "query larger than evals");
		BN_REQUIRE(jb.n_terms <= BN_PEL_MAX_TERMS, "partial eval: too many terms in a job");
		BN_REQUIRE(jb.first_term <= n_terms_total && jb.n_terms <= n_terms_total - jb.first_term, "partial eval: a job's terms leave the term table");
		for (uint32_t t = jb.first_term; t < jb.first_term + jb.n_terms; t++) {
			BN_REQUIRE(jb.n_vars + terms[t].tower_level >= 7, "partial eval: a column is at least one 128-bit element");
			ranges.push_back(pel_range{(uintptr_t)terms[t].d_evals, (uintptr_t)terms[t].d_evals + 16 * (uintptr_t)column_elems(jb.n_vars, terms[t].tower_level), false});
		}
		ranges.push_back(pel_range{(uintptr_t)d_outs[j], (uintptr_t)d_outs[j] + ((uintptr_t)16 << (jb.n_vars - q)), true});
	}
	// an output overlaps neither an input nor another output (inputs may overlap each other): one sweep over the sorted ranges
	std::sort(ranges.begin(), ranges.end(), [](const pel_range &x, const pel_range &y) { return x.begin < y.begin; });
	uintptr_t end_in = 0, end_out = 0;
	for (const pel_range &r : ranges) {
		BN_REQUIRE(r.begin >= end_out && (!r.output || r.begin >= end_in), "partial eval: an output overlaps a column, the query or another output");
		(r.output ? end_out : end_in) = std::max(r.output ? end_out : end_in, r.end);
	}

	// ---- the classes of every job
	std::vector<bn::pel_class> classes;
	std::vector<const uint64_t *> cols;
	std::vector<bn::pel_job> small, wide, init;
	struct shape {
		uint32_t max_level;
		bool has_bits;
	};
	std::vector<shape> shapes; // of `small`
	bool bits_one = true;
	uint32_t lds_out = 0;
	uint64_t wide_units = 0;
	for (uint32_t j = 0; j < n_jobs; j++) {
		const bn_pel_job &jb = jobs[j];
		std::vector<uint32_t> order;
		for (uint32_t t = jb.first_term; t < jb.first_term + jb.n_terms; t++)
			if (terms[t].coeff.lo | terms[t].coeff.hi) order.push_back(t); // (a zero coefficient contributes nothing)
		auto key_less = [&](uint32_t x, uint32_t y) {
			const bn_pel_term &a = terms[x], &c = terms[y];
			if (a.tower_level != c.tower_level) return a.tower_level < c.tower_level;
			if (a.coeff.hi != c.coeff.hi) return a.coeff.hi < c.coeff.hi;
			return a.coeff.lo < c.coeff.lo;
		};
		std::stable_sort(order.begin(), order.end(), key_less);
		const uint32_t b = jb.n_vars - q, first_class = (uint32_t)classes.size();
		shape sh{0, false};
		for (size_t at = 0; at < order.size();) {
			size_t end = at;
			while (end < order.size() && !key_less(order[at], order[end])) end++;
			const bn_pel_term &t0 = terms[order[at]];
			const bool one = t0.coeff.lo == 1 && t0.coeff.hi == 0;
			classes.push_back(bn::pel_class{f128{t0.coeff.lo, t0.coeff.hi}, (uint32_t)cols.size(), (uint32_t)(end - at), t0.tower_level, one ? 1u : 0u});
			for (size_t i = at; i < end; i++) cols.push_back((const uint64_t *)terms[order[i]].d_evals);
			sh.max_level = std::max(sh.max_level, t0.tower_level);
			sh.has_bits = sh.has_bits || t0.tower_level == 0;
			at = end;
		}
		const uint32_t n_classes = (uint32_t)classes.size() - first_class;
		bn::pel_job pj{f128{jb.offset.lo, jb.offset.hi}, (uint64_t *)d_outs[j], first_class, n_classes, b, 0, 0, 0};
		if (b > bn::kPeMaxLogOut) {
			BN_REQUIRE(wide_units + ((uint64_t)1 << (b - 8)) < (1ull << 31), "partial eval: batch too large for one call");
			pj.start = (uint32_t)wide_units;
			wide_units += (uint64_t)1 << (b - 8);
			wide.push_back(pj);
			continue;
		}
		init.push_back(pj);
		if (n_classes == 0) continue; // (the offset alone: k_pel_init's work)
		for (uint32_t c = first_class; c < classes.size(); c++) bits_one = bits_one && classes[c].level == 0 && classes[c].one;
		lds_out = std::max(lds_out, 1u << b);
		small.push_back(pj);
		shapes.push_back(sh);
	}
	uint64_t units = 0, max_share = 0;
	for (uint32_t shrink = 0; shrink < 3; shrink++) {
		units = 0;
		max_share = 0;
		for (size_t i = 0; i < small.size(); i++) {
			small[i].log_ch = pel_log_ch(shapes[i].max_level, shapes[i].has_bits, small[i].b, q, shrink);
			const uint64_t n_chunks = (uint64_t)1 << (q - small[i].log_ch);
			BN_REQUIRE(units + n_chunks < (1ull << 31), "partial eval: batch too large for one call");
			small[i].start = (uint32_t)units;
			units += n_chunks;
			max_share = std::max(max_share, n_chunks);
		}
		if (units >= (uint64_t)ctx->n_cu * 4) break;
	}

	// ---- one upload: [init jobs][unit jobs][wide jobs][classes][column pointers]
	call_upload up(ctx);
	const auto s_init = up.reserve<bn::pel_job>(init.size());
	const auto s_small = up.reserve<bn::pel_job>(small.size());
	const auto s_wide = up.reserve<bn::pel_job>(wide.size());
	const auto s_classes = up.reserve<bn::pel_class>(classes.size());
	const auto s_cols = up.reserve<const uint64_t *>(cols.size());
	if (const int rc = up.alloc()) return rc;
	std::copy(init.begin(), init.end(), up.host(s_init));
	std::copy(small.begin(), small.end(), up.host(s_small));
	std::copy(wide.begin(), wide.end(), up.host(s_wide));
	std::copy(classes.begin(), classes.end(), up.host(s_classes));
	std::copy(cols.begin(), cols.end(), up.host(s_cols));
	BN_HIP(up.send());
	BN_HIP(bn::launch_partial_eval_lincomb(ctx->stream, up.dev(s_init), (uint32_t)init.size(), up.dev(s_small), (uint32_t)small.size(), up.dev(s_classes),
	                                       up.dev(s_cols), d_tensor_query, (uint32_t)units, lds_out, bits_one));
	BN_HIP(bn::launch_partial_eval_lincomb_wide(ctx->stream, up.dev(s_wide), (uint32_t)wide.size(), up.dev(s_classes), up.dev(s_cols), d_tensor_query, q,
	                                            (uint32_t)wide_units));
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the outputs are complete when the call returns; the tables are pageable host memory that goes out of scope)
	// (a call that failed on the way counts nowhere)
	ctx->pel_calls++;
	ctx->pel_launches += (init.empty() ? 0 : 2) + (wide.empty() ? 0 : 1); // k_pel_init + k_pel, k_pel_wide
	ctx->pel_jobs += n_jobs;
	for (uint32_t j = 0; j < n_jobs; j++) ctx->pel_terms += jobs[j].n_terms;
	ctx->pel_classes += classes.size();
	ctx->pel_jobs_fallback += wide.size();
	ctx->pel_max_share = max_share;
	return BN_OK;
}

int bn_partial_eval_lincomb_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_PEL_CALLS] = ctx->pel_calls;
	counters[BN_PEL_LAUNCHES] = ctx->pel_launches;
	counters[BN_PEL_JOBS] = ctx->pel_jobs;
	counters[BN_PEL_TERMS] = ctx->pel_terms;
	counters[BN_PEL_CLASSES] = ctx->pel_classes;
	counters[BN_PEL_JOBS_FALLBACK] = ctx->pel_jobs_fallback;
	counters[BN_PEL_MAX_SHARE] = ctx->pel_max_share;
	return BN_OK;
}

} // extern "C"
