// binius_amd/csrc/abi_generate.cpp -- bn_generate_columns_batch: the Projected columns at a hypercube vertex (m3's add_selected /
// add_projected; math/src/multilinear_extension.rs:193-237), the Constant, StepDown, StepUp, SelectRow and Powers transparents
// (core/src/transparent/) and the incrementing column (m3/src/builder/structured.rs:64-81) written on the device.  Argument validation
// and the plan of the launch; the kernel is in kernels_generate.hip.
//
// The plan: every job becomes one form of the kernel (internal.hpp, generate_job) with its parameters in bit coordinates -- a value
// of tower level l is 2^l bits, a run of a projection 2^(start_index + l) bits at a stride of 2^(start_index + query_size + l) -- and is
// cut into units of kGenerateUnitElems output elements (kGeneratePieceUnitElems where an element is made of several input elements or of field products).
// One upload carries the job table and the power table (base^(2^b), by squaring with the host product); one launch serves them all.
#include <algorithm>

#include "abi_common.hpp"
#include "hostmul.hpp"

namespace {

struct gn_range {
	uintptr_t begin, end;
	bool output;
};

// the pattern of `bits` (a power of two, at most 64) bits repeated through a 64-bit word
uint64_t gn_repeat(uint64_t pattern, uint32_t bits)
{
	if (bits < 64) pattern &= ((uint64_t)1 << bits) - 1;
	for (uint32_t b = bits; b < 64; b <<= 1) pattern |= pattern << b;
	return pattern;
}
// a value of the level: below 2^(2^level)
bool gn_in_level(const bn_f128 &v, uint32_t l) { return l == 7 || (v.hi == 0 && (l == 6 || v.lo < ((uint64_t)1 << (1u << l)))); }

} // namespace

extern "C" {

int bn_generate_columns_batch(bn_ctx *ctx, const void *jobs_, uint32_t n_jobs)
{
	const bn_generate_job *jobs = (const bn_generate_job *)jobs_;
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	if (n_jobs == 0) return BN_OK;
	BN_REQUIRE(jobs, "null argument");
	BN_REQUIRE(n_jobs <= (1u << 20), "too many jobs for one call");
	std::vector<gn_range> ranges;
	std::vector<bn::generate_job> table;
	std::vector<bn::f128> powers;
	uint64_t units = 0;
	for (uint32_t j = 0; j < n_jobs; j++) {
		const bn_generate_job &jb = jobs[j];
		const uint32_t l = jb.tower_level, n = jb.n_vars;
		BN_REQUIRE(jb.kind <= BN_GEN_POWERS, "generate: unknown kind");
		BN_REQUIRE(l <= 7, "generate: tower_level > 7");
		BN_REQUIRE(valid_tower_level(l), "unsupported value of tower_level");
		BN_REQUIRE(jb.reserved == 0, "generate: reserved must be 0");
		BN_REQUIRE(n <= BN_PE_MAX_VARS, "generate: a column has at most 2^40 values");
		BN_REQUIRE(n + l >= 7, "generate: an output is at least one 128-bit element");
		BN_REQUIRE(jb.d_out, "generate: null pointer");
		BN_REQUIRE(aligned16(jb.d_out), "generate: pointers must be 16-byte aligned");
		bn::generate_job d{};
		d.out = (uint4 *)jb.d_out;
		d.out_elems = (uint64_t)1 << (n + l - 7);
		switch (jb.kind) {
		case BN_GEN_PROJECTED_BITS: {
			BN_REQUIRE(jb.d_inner, "generate: null pointer");
			BN_REQUIRE(aligned16(jb.d_inner), "generate: pointers must be 16-byte aligned");
			BN_REQUIRE(jb.query_size >= 1 && jb.query_size <= BN_PE_MAX_VARS - n, "generate: query_size outside 1 .. BN_PE_MAX_VARS - n_vars");
			BN_REQUIRE(jb.query_bits < ((uint64_t)1 << jb.query_size), "generate: query_bits >= 2^query_size");
			BN_REQUIRE(jb.start_index <= n, "generate: start_index + query_size > inner_n_vars");
			const uint32_t w = jb.start_index + l, W = w + jb.query_size; // log2 of a run and of the stride, in bits
			d.in = jb.d_inner;
			if (w >= 7) {
				d.form = bn::kGnProjElem;
				d.p0 = w - 7;
				d.p1 = W - 7;
				d.m0 = jb.query_bits << (w - 7);
			} else if (W >= 7) {
				const uint64_t at = jb.query_bits << w; // bit of a stride where its run starts
				d.form = bn::kGnProjField;
				d.p0 = w;
				d.p1 = W - 7;
				d.p2 = (uint32_t)(at & 127);
				d.m0 = at >> 7;
			} else {
				d.form = bn::kGnProjSpread;
				d.p0 = w;
				d.p1 = W;
				d.p2 = jb.query_size;
				d.p3 = (uint32_t)(jb.query_bits << w);
			}
			ranges.push_back(gn_range{(uintptr_t)jb.d_inner, (uintptr_t)jb.d_inner + 16 * (uintptr_t)column_elems(n + jb.query_size, l), false});
			break;
		}
		case BN_GEN_CONSTANT: {
			BN_REQUIRE(gn_in_level(jb.value, l), "generate: the value is a value of the output's tower level");
			d.form = bn::kGnConst;
			d.m0 = l == 7 ? jb.value.lo : gn_repeat(jb.value.lo, 1u << l);
			d.m1 = l == 7 ? jb.value.hi : d.m0;
			break;
		}
		case BN_GEN_STEP_DOWN:
		case BN_GEN_STEP_UP: {
			BN_REQUIRE(l == 0, "generate: a step column is a B1 column");
			BN_REQUIRE(jb.index <= ((uint64_t)1 << n), "generate: index > 2^n_vars");
			d.form = bn::kGnStep;
			d.m0 = jb.index;
			d.m1 = jb.kind == BN_GEN_STEP_UP ? ~(uint64_t)0 : 0;
			break;
		}
		case BN_GEN_SELECT_ROW: {
			BN_REQUIRE(l == 0, "generate: a select-row column is a B1 column");
			BN_REQUIRE(jb.index < ((uint64_t)1 << n), "generate: index >= 2^n_vars");
			d.form = bn::kGnSelect;
			d.m0 = jb.index;
			break;
		}
		case BN_GEN_INCREMENTING: {
			BN_REQUIRE(n <= (1u << l), "generate: an incrementing column has n_vars <= 2^tower_level");
			d.form = bn::kGnIncrement;
			d.p0 = 1u << l;
			if (l < 7) {
				d.p1 = 6 - l;
				for (uint32_t t = 0; t < (64u >> l); t++) d.m0 |= (uint64_t)t << (t << l); // the values 0, 1, ... of a word at their places
			}
			break;
		}
		default: {
			BN_REQUIRE(l >= 3, "generate: a column of powers has tower level 3 .. 7");
			BN_REQUIRE(gn_in_level(jb.value, l), "generate: the base is a value of the output's tower level");
			d.form = bn::kGnPowers;
			d.p0 = l;
			d.p1 = n;
			d.table = (uint32_t)powers.size();
			bn::f128 p{jb.value.lo, jb.value.hi};
			for (uint32_t b = 0; b < bn::kGeneratePowerEntries; b++) {
				powers.push_back(p);
				p = bn::mul_host(p, p);
			}
			break;
		}
		}
		d.unit_elems = d.form == bn::kGnProjField || d.form == bn::kGnProjSpread || d.form == bn::kGnPowers ? bn::kGeneratePieceUnitElems : bn::kGenerateUnitElems;
		const uint64_t n_units = (d.out_elems + d.unit_elems - 1) / d.unit_elems;
		BN_REQUIRE(units + n_units < (1ull << 31), "generate: batch too large for one call");
		d.start = (uint32_t)units;
		units += n_units;
		table.push_back(d);
		ranges.push_back(gn_range{(uintptr_t)jb.d_out, (uintptr_t)jb.d_out + 16 * (uintptr_t)d.out_elems, true});
	}
	// an output overlaps neither an inner column of any job nor another output (inner columns may overlap each other): one sweep over
	// the sorted ranges
	std::sort(ranges.begin(), ranges.end(), [](const gn_range &x, const gn_range &y) { return x.begin < y.begin; });
	uintptr_t end_in = 0, end_out = 0;
	for (const gn_range &r : ranges) {
		BN_REQUIRE(r.begin >= end_out && (!r.output || r.begin >= end_in), "generate: an output overlaps an inner column or another output");
		(r.output ? end_out : end_in) = std::max(r.output ? end_out : end_in, r.end);
	}
	BN_FLUSH(ctx);

	// ---- one upload: [jobs][powers]
	call_upload up(ctx);
	const auto s_jobs = up.reserve<bn::generate_job>(table.size());
	const auto s_powers = up.reserve<bn::f128>(powers.size());
	if (const int rc = up.alloc()) return rc;
	std::copy(table.begin(), table.end(), up.host(s_jobs));
	std::copy(powers.begin(), powers.end(), up.host(s_powers));
	BN_HIP(up.send());
	BN_HIP(bn::launch_generate_columns(ctx->stream, up.dev(s_jobs), n_jobs, up.dev(s_powers), (uint32_t)units));
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the outputs are complete when the call returns; the tables are pageable host memory that goes out of scope)
	ctx->gn_calls++;
	ctx->gn_launches++;
	ctx->gn_jobs += n_jobs;
	return BN_OK;
}

int bn_generate_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_GENERATE_CALLS] = ctx->gn_calls;
	counters[BN_GENERATE_LAUNCHES] = ctx->gn_launches;
	counters[BN_GENERATE_JOBS] = ctx->gn_jobs;
	return BN_OK;
}

} // extern "C"
