// binius_amd/csrc/abi_derive.cpp -- bn_derive_columns_batch: the Shifted, Repeating, ZeroPadded and unit-coefficient LinearCombination
// columns of a constraint system (multilinear.rs of core's oracle module; constraint_system/validate.rs:151-279; math/src/fold.rs:27-77) built on
// the device from the columns they are functions of.  Argument validation and the plan of the launch; the kernel is in
// kernels_derive.hip.
//
// The plan: every job becomes one form of the kernel (internal.hpp, derive_job) with its parameters in bit coordinates -- a value of
// tower level l is 2^l bits, a block of a shift 2^(block_size + l) bits -- and is cut into units of kDeriveUnitElems output elements.
// One upload carries the job table and the term pointers; one launch serves them all.
#include <algorithm>

#include "abi_common.hpp"

namespace {

struct dv_range {
	uintptr_t begin, end;
	bool output;
};

// the pattern of `bits` (a power of two, at most 64) bits repeated through a 64-bit word
uint64_t dv_repeat(uint64_t pattern, uint32_t bits)
{
	if (bits < 64) pattern &= ((uint64_t)1 << bits) - 1;
	for (uint32_t b = bits; b < 64; b <<= 1) pattern |= pattern << b;
	return pattern;
}
uint64_t dv_low_bits(uint32_t n) { return n >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << n) - 1; }

} // namespace

extern "C" {

int bn_derive_columns_batch(bn_ctx *ctx, const void *jobs_, uint32_t n_jobs, const void *const *d_terms, uint32_t n_terms_total)
{
	const bn_derive_job *jobs = (const bn_derive_job *)jobs_;
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	if (n_jobs == 0) return BN_OK;
	BN_REQUIRE(jobs && (d_terms || n_terms_total == 0), "null argument");
	BN_REQUIRE(n_jobs <= (1u << 20), "too many jobs for one call");
	for (uint32_t t = 0; t < n_terms_total; t++) {
		BN_REQUIRE(d_terms[t], "derive: null pointer");
		BN_REQUIRE(aligned16(d_terms[t]), "derive: pointers must be 16-byte aligned");
	}
	std::vector<dv_range> ranges;
	std::vector<bn::derive_job> table;
	uint64_t units = 0;
	auto input = [&](const void *p, uint32_t n_vars, uint32_t level) {
		ranges.push_back(dv_range{(uintptr_t)p, (uintptr_t)p + 16 * (uintptr_t)column_elems(n_vars, level), false});
	};
	for (uint32_t j = 0; j < n_jobs; j++) {
		const bn_derive_job &jb = jobs[j];
		const uint32_t l = jb.tower_level, n = jb.n_vars;
		BN_REQUIRE(jb.kind <= BN_DERIVE_XOR_COMBINATION, "derive: unknown kind");
		BN_REQUIRE(l <= 7, "derive: tower_level > 7");
		BN_REQUIRE(valid_tower_level(l), "unsupported value of tower_level");
		BN_REQUIRE(jb.reserved == 0, "derive: reserved must be 0");
		BN_REQUIRE(n <= BN_PE_MAX_VARS, "derive: a column has at most 2^40 values");
		BN_REQUIRE(n + l >= 7, "derive: an output is at least one 128-bit element");
		BN_REQUIRE(jb.d_out, "derive: null pointer");
		BN_REQUIRE(aligned16(jb.d_out), "derive: pointers must be 16-byte aligned");
		if (jb.kind != BN_DERIVE_XOR_COMBINATION) {
			BN_REQUIRE(jb.d_inner, "derive: null pointer");
			BN_REQUIRE(aligned16(jb.d_inner), "derive: pointers must be 16-byte aligned");
		}
		const uint32_t log_elems = n + l - 7;
		bn::derive_job d{};
		d.in = jb.d_inner;
		d.out = (uint4 *)jb.d_out;
		d.out_elems = (uint64_t)1 << log_elems;
		switch (jb.kind) {
		case BN_DERIVE_SHIFTED: {
			BN_REQUIRE(jb.shift_variant <= BN_SHIFT_LOGICAL_RIGHT, "derive: unknown shift variant");
			BN_REQUIRE(jb.block_size <= n, "derive: block_size > n_vars");
			BN_REQUIRE(jb.shift_offset >= 1 && jb.shift_offset < ((uint64_t)1 << jb.block_size), "derive: shift_offset outside 1 .. 2^block_size - 1");
			const uint32_t log_block = jb.block_size + l; // bits
			const uint64_t s = jb.shift_offset << l;
			const bool right = jb.shift_variant == BN_SHIFT_LOGICAL_RIGHT, circular = jb.shift_variant == BN_SHIFT_CIRCULAR_LEFT;
			if (log_block <= 6) {
				const uint32_t B = 1u << log_block;
				const uint64_t low_s = dv_repeat(dv_low_bits((uint32_t)s), B), low_rest = dv_repeat(dv_low_bits(B - (uint32_t)s), B);
				d.form = bn::kDvShiftWord;
				if (!right) { // positions s .. B - 1 of a block take the word moved up by s
					d.p0 = (uint32_t)s;
					d.m0 = ~low_s;
				}
				if (circular) { // positions 0 .. s - 1 take what left the block at its top
					d.p1 = B - (uint32_t)s;
					d.m1 = low_s;
				}
				if (right) {
					d.p1 = (uint32_t)s;
					d.m1 = low_rest;
				}
			} else {
				const uint64_t block = (uint64_t)1 << log_block, delta = right ? s : block - s; // out[o] = in[o + delta] before the block's wrap
				d.form = bn::kDvShiftElem;
				d.p0 = log_block - 7;
				d.p1 = circular ? 1 : 0;
				d.p2 = (uint32_t)(delta & 127);
				d.m0 = delta >> 7;
				d.m1 = right ? 0 : block >> 7; // logical left: o + delta - block must not be negative
			}
			input(jb.d_inner, n, l);
			break;
		}
		case BN_DERIVE_REPEATING: {
			BN_REQUIRE(jb.inner_n_vars <= n, "derive: inner_n_vars > n_vars");
			const uint32_t log_in = jb.inner_n_vars + l;
			d.form = bn::kDvRepeat;
			d.m0 = log_in >= 7 ? ((uint64_t)1 << (log_in - 7)) - 1 : 0;
			d.p0 = log_in >= 7 ? 0 : 1u << log_in;
			input(jb.d_inner, jb.inner_n_vars, l);
			break;
		}
		case BN_DERIVE_ZERO_PADDED: {
			BN_REQUIRE(jb.inner_n_vars <= n, "derive: inner_n_vars > n_vars");
			const uint32_t pad = n - jb.inner_n_vars;
			BN_REQUIRE(jb.start_index <= jb.inner_n_vars, "IncorrectStartIndex: start_index > inner_n_vars");
			BN_REQUIRE(jb.nonzero_index < ((uint64_t)1 << pad), "IncorrectNonZeroIndex: nonzero_index >= 2^n_pad_vars");
			const uint32_t log_run = jb.start_index + l, log_period = log_run + pad; // bits
			if (log_run >= 7) {
				d.form = bn::kDvPadElem;
				d.p0 = log_run - 7;
				d.p1 = log_period - 7;
				d.m0 = jb.nonzero_index;
			} else if (log_period >= 7) {
				const uint64_t at = jb.nonzero_index << log_run; // bit of a period where its run starts
				d.form = bn::kDvPadField;
				d.p0 = log_run;
				d.p1 = log_period - 7;
				d.p2 = (uint32_t)(at & 127);
				d.m0 = at >> 7;
			} else {
				d.form = bn::kDvPadSpread;
				d.p0 = log_run;
				d.p1 = log_period;
				d.p2 = pad;
				d.p3 = (uint32_t)(jb.nonzero_index << log_run);
			}
			input(jb.d_inner, jb.inner_n_vars, l);
			break;
		}
		default: {
			BN_REQUIRE(jb.n_terms <= BN_PEL_MAX_TERMS, "derive: too many terms in a job");
			BN_REQUIRE(jb.first_term <= n_terms_total && jb.n_terms <= n_terms_total - jb.first_term, "derive: a job's terms leave the term list");
			BN_REQUIRE(l == 7 || (jb.offset.hi == 0 && (l == 6 || jb.offset.lo < ((uint64_t)1 << (1u << l)))), "derive: the offset is a value of the output's tower level");
			d.form = bn::kDvXor;
			d.in = nullptr;
			d.first_term = jb.first_term;
			d.n_terms = jb.n_terms;
			d.m0 = l == 7 ? jb.offset.lo : dv_repeat(jb.offset.lo, 1u << l);
			d.m1 = l == 7 ? jb.offset.hi : d.m0;
			for (uint32_t t = jb.first_term; t < jb.first_term + jb.n_terms; t++) input(d_terms[t], n, l);
			break;
		}
		}
		const uint64_t n_units = (d.out_elems + bn::kDeriveUnitElems - 1) / bn::kDeriveUnitElems;
		BN_REQUIRE(units + n_units < (1ull << 31), "derive: batch too large for one call");
		d.start = (uint32_t)units;
		units += n_units;
		table.push_back(d);
		ranges.push_back(dv_range{(uintptr_t)jb.d_out, (uintptr_t)jb.d_out + 16 * (uintptr_t)d.out_elems, true});
	}
	// an output overlaps neither an input of any job nor another output (inputs may overlap each other): one sweep over the sorted ranges
	std::sort(ranges.begin(), ranges.end(), [](const dv_range &x, const dv_range &y) { return x.begin < y.begin; });
	uintptr_t end_in = 0, end_out = 0;
	for (const dv_range &r : ranges) {
		BN_REQUIRE(r.begin >= end_out && (!r.output || r.begin >= end_in), "derive: an output overlaps an inner column, a term or another output");
		(r.output ? end_out : end_in) = std::max(r.output ? end_out : end_in, r.end);
	}
	BN_FLUSH(ctx);

	// ---- one upload: [jobs][term pointers]
	call_upload up(ctx);
	const auto s_jobs = up.reserve<bn::derive_job>(table.size());
	const auto s_terms = up.reserve<const void *>(n_terms_total);
	if (const int rc = up.alloc()) return rc;
	std::copy(table.begin(), table.end(), up.host(s_jobs));
	std::copy(d_terms, d_terms + n_terms_total, up.host(s_terms));
	BN_HIP(up.send());
	BN_HIP(bn::launch_derive_columns(ctx->stream, up.dev(s_jobs), n_jobs, up.dev(s_terms), (uint32_t)units));
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the outputs are complete when the call returns; the tables are pageable host memory that goes out of scope)
	ctx->dv_calls++;
	ctx->dv_launches++;
	ctx->dv_jobs += n_jobs;
	return BN_OK;
}

int bn_derive_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_DERIVE_CALLS] = ctx->dv_calls;
	counters[BN_DERIVE_LAUNCHES] = ctx->dv_launches;
	counters[BN_DERIVE_JOBS] = ctx->dv_jobs;
	return BN_OK;
}

} // extern "C"
