// binius_amd/host/evalcheck.hpp -- C++ mirror of one round of evalcheck's bivariate sumchecks: one call of
// prove_bivariate_sumchecks_with_switchover (core/src/protocols/evalcheck/subclaims.rs:549-586) together with the witness
// construction in front of it:
//
//   process_shifted_sumcheck / process_packed_sumcheck   subclaims.rs:52-145     the constraint sets: inner projection x shift indicator,
//                                                                                 inner projection x tower basis, over b variables
//   collect_projected_mles                               subclaims.rs:356-439    evaluate_partial_high of every inner column at the high
//                                                                                 coordinates of its claim -> ONE bn_partial_eval_high_batch
//                                                                                 per distinct suffix
//   try_build_partial_eval                               subclaims.rs:305-346    an inner column that is a LinearCombination: projected from
//                                                                                 its constituents, never materialised -> ONE
//                                                                                 bn_partial_eval_high_lincomb_batch per distinct suffix
//   ShiftIndPartialEval::multilinear_extension           transparent/shift_ind.rs:117-161, 276-366   host table of 2^b elements
//   TowerBasis::multilinear_extension                    transparent/tower_basis.rs:54-70            host table of 2^k elements
//   RegularSumcheckProver per constraint set + batch_prove   -> BivariateSumcheckProver + SumcheckBatchProver (sumcheck.hpp, batch_prover.hpp):
//     both batch a prover's claims by powers of the batch coefficient (prover_state.rs:302) and the round polynomial is unique,
//     so the transcript is the same.  At 2^b <= 2^12 elements the backend's host tail finishes these provers.
//
// The caller hands in explicit multilinear lists (the order its constraint set holds them = the order of the final evaluations
// in the transcript); the oracle-set bookkeeping of EvalcheckProver stays with the caller.
//
// What comes out: the truncated round proofs and the final evaluations in finishing order.  A PROJECTION's final evaluation v at
// the reversed challenges r' (r'[i] = the challenge of round b - 1 - i of its prover) is the new evalcheck claim (r' || suffix, v)
// on its inner column (for a LINCOMB: on the linear-combination oracle itself); a shift indicator's or tower basis's final evaluation
// is what the verifier recomputes itself.
//
// evalcheck_evaluate_claims is the step in FRONT of every round: EvalcheckProver::prove evaluates the materialised witness of every leaf
// oracle whose value is not yet known at its whole claim point ("MLE Fold Full", evalcheck/prove.rs:191-275, make_new_eval_claim :812-879).
// The reference splits the point in the middle, reuses an already memoised suffix when it has one (:211-221), takes evaluate_partial_high
// at the suffix and evaluates the result at the prefix.  The arithmetic is exact, so the value does not depend on where the point is
// split: the mirror splits at min(|point| / 2, kEvalcheckLoSplit), the split the device op is fastest at, and does not reproduce the
// reference's middle split or its suffix reuse.  Handing the per-(column, suffix) partial evaluations on to collect_projected_mles
// stays out of scope.
//
// Protocol bookkeeping only: every hypercube-sized operation is a call of the backend.
#pragma once
#include <algorithm>
#include <map>
#include <memory>

#include "batch_prover.hpp"

namespace binius_amd {

enum class ShiftVariant : uint32_t { CircularLeft = 0, LogicalLeft = 1, LogicalRight = 2 };

struct EvalcheckMultilinear {
	enum Kind : uint32_t { Projection = 0, ShiftInd = 1, TowerBasis = 2, LinComb = 3 } kind = Projection;
	// Projection: the inner column (2^n_vars values of tower_level, packed into F, only read) at the suffix pool[suffix_off .. + suffix_len)
	const void *d_column = nullptr;
	uint32_t tower_level = 0, n_vars = 0;
	uint32_t suffix_off = 0, suffix_len = 0;
	// ShiftInd: (block_size, shift_offset, variant) at the prefix pool[r_off .. + block_size)
	uint32_t block_size = 0, shift_offset = 0;
	ShiftVariant variant = ShiftVariant::CircularLeft;
	uint32_t r_off = 0, r_len = 0;
	// TowerBasis: table[i] = basis(iota, i), i < 2^k
	uint32_t k = 0, iota = 0;
	// LinComb: offset + sum of coeff * column over the terms [first_term, first_term + n_terms) of the call's term list (nested combinations
	// flattened by the caller), 2^n_vars values each, at the suffix pool[suffix_off .. + suffix_len)
	uint32_t first_term = 0, n_terms = 0;
	B128 offset = B128::ZERO();
};

// one constituent of a linear combination: a column as it is read (2^n_vars values of tower_level, packed into F) and its coefficient
struct EvalcheckTerm {
	const void *d_column = nullptr;
	uint32_t tower_level = 0;
	B128 coeff = B128::ONE();
};

struct EvalcheckProver {
	size_t n_vars = 0; // b
	std::vector<EvalcheckMultilinear> multilins;
	std::vector<IndexCompositionBivariate> compositions;
	std::vector<B128> sums;
};

// the identity of a suffix: its slice of the pool
using EvalcheckSuffix = std::pair<uint32_t, uint32_t>;
// the identity of a projection: the column as it is read (pointer, tower level; n_vars follows from b and the suffix) and the suffix
using EvalcheckProjection = std::pair<std::pair<const void *, uint32_t>, EvalcheckSuffix>;
inline EvalcheckProjection evalcheck_projection_key(const EvalcheckMultilinear &m)
{
	return {{m.d_column, m.tower_level}, {m.suffix_off, m.suffix_len}};
}

// the identity of a linear-combination projection: (term range, offset, suffix) and the number of variables the terms are read with
using EvalcheckLinComb = std::pair<std::pair<std::pair<uint32_t, uint32_t>, std::pair<uint64_t, uint64_t>>, std::pair<EvalcheckSuffix, uint32_t>>;
inline EvalcheckLinComb evalcheck_lincomb_key(const EvalcheckMultilinear &m)
{
	return {{{m.first_term, m.n_terms}, {m.offset.lo, m.offset.hi}}, {{m.suffix_off, m.suffix_len}, m.n_vars}};
}

// Exact: the tensor expansion of every distinct suffix, one table per distinct (column, tower level, suffix) projection, per distinct
// (term range, offset, suffix) linear combination and per transparent multilinear, and the provers' fold buffers (m * 2^(b-1) each).
inline size_t evalcheck_scratch_elems(const std::vector<EvalcheckProver> &provers)
{
	std::map<EvalcheckSuffix, bool> suffixes;
	std::map<EvalcheckProjection, bool> projections;
	std::map<EvalcheckLinComb, bool> lincombs;
	size_t total = 0;
	for (const EvalcheckProver &p : provers) {
		for (const EvalcheckMultilinear &m : p.multilins) {
			if (m.kind == EvalcheckMultilinear::Projection) {
				const EvalcheckSuffix s{m.suffix_off, m.suffix_len};
				if (suffixes.emplace(s, true).second) total += (size_t)1 << m.suffix_len;
				if (projections.emplace(evalcheck_projection_key(m), true).second) total += (size_t)1 << p.n_vars;
			} else if (m.kind == EvalcheckMultilinear::LinComb) {
				const EvalcheckSuffix s{m.suffix_off, m.suffix_len};
				if (suffixes.emplace(s, true).second) total += (size_t)1 << m.suffix_len;
				if (lincombs.emplace(evalcheck_lincomb_key(m), true).second) total += (size_t)1 << p.n_vars;
			} else {
				total += (size_t)1 << p.n_vars;
			}
		}
		if (p.n_vars >= 1) total += p.multilins.size() << (p.n_vars - 1);
	}
	return total;
}

// ShiftIndPartialEval::multilinear_extension (shift_ind.rs:117-161, 332-366): table[x] = sum_y f(x, y) eq(y, r) with f(x, y) = 1 where
// y is the position x is shifted to -- table[x] = eq(r)[y(x)], zero where the shift leaves the block
inline std::vector<B128> evalcheck_shift_ind_table(size_t b, size_t offset, ShiftVariant variant, const B128 *r)
{
	// assert_valid_shift_ind_args (shift_ind.rs:218-235)
	if (b == 0 || b >= 32) throw Error(Error::InputValidation, "shift indicator: block_size out of range");
	const size_t n = (size_t)1 << b;
	if (offset == 0 || offset >= n) throw Error(Error::InputValidation, "shift indicator: shift_offset must be in 1 .. 2^block_size - 1");
	const std::vector<B128> eq = eq_expand(r, b);
	std::vector<B128> table(n, B128::ZERO());
	for (size_t x = 0; x < n; x++) {
		switch (variant) {
		case ShiftVariant::CircularLeft: table[x] = eq[(x + offset) & (n - 1)]; break;
		case ShiftVariant::LogicalLeft:
			if (x + offset < n) table[x] = eq[x + offset];
			break;
		case ShiftVariant::LogicalRight:
			if (x >= offset) table[x] = eq[x - offset];
			break;
		}
	}
	return table;
}

// per round the truncated coefficients; per prover, in finishing (= input) order, its final evaluations
using EvalcheckOutput = BatchSumcheckOutput;

// Schedule (subclaims.rs:549-586 = front_loaded::BatchProver::new + run): sample the n_provers batch coefficients (stream
// EvalcheckBatchCoeffs); per round the evaluations of the provers that finished, the truncated round polynomial (2 coefficients),
// ONE sample (stream EvalcheckChallenges); after the last round the evaluations of the provers that finish then.
enum { EvalcheckBatchCoeffs = 0, EvalcheckChallenges = 1 };
inline EvalcheckOutput evalcheck_bivariate_prove(ComputeLayer &hal, const std::vector<EvalcheckProver> &provers, const std::vector<B128> &pool, FSliceMut scratch,
                                                 TranscriptSource &tr, const std::vector<EvalcheckTerm> &terms = {})
{
	size_t total_m = 0;
	for (size_t i = 0; i < provers.size(); i++) {
		const EvalcheckProver &p = provers[i];
		if (p.n_vars > 12) throw Error(Error::InputValidation, "a prover of an evalcheck round has at most 12 variables");
		if (i && p.n_vars < provers[i - 1].n_vars) throw Error(Error::InputValidation, "ClaimsOutOfOrder: provers ascend by number of variables");
		if (p.compositions.size() != p.sums.size()) throw Error(Error::InputValidation, "one sum per claim");
		for (const EvalcheckMultilinear &m : p.multilins) {
			switch (m.kind) {
			case EvalcheckMultilinear::Projection:
				if (!m.d_column) throw Error(Error::InputValidation, "null inner column");
				if (m.n_vars != p.n_vars + m.suffix_len) throw Error(Error::InputValidation, "a projection's inner column has b + |suffix| variables");
				if ((size_t)m.suffix_off + m.suffix_len > pool.size()) throw Error(Error::InputValidation, "a suffix leaves the point pool");
				break;
			case EvalcheckMultilinear::LinComb:
				if (m.n_vars != p.n_vars + m.suffix_len) throw Error(Error::InputValidation, "a linear combination has b + |suffix| variables");
				if ((size_t)m.suffix_off + m.suffix_len > pool.size()) throw Error(Error::InputValidation, "a suffix leaves the point pool");
				if ((size_t)m.first_term + m.n_terms > terms.size()) throw Error(Error::InputValidation, "a linear combination's terms leave the term list");
				break;
			case EvalcheckMultilinear::ShiftInd:
				if (m.block_size != p.n_vars || m.r_len != m.block_size) throw Error(Error::InputValidation, "shift indicator: block_size and |r| must equal the prover's number of variables");
				if ((size_t)m.r_off + m.r_len > pool.size()) throw Error(Error::InputValidation, "a shift indicator's prefix leaves the point pool");
				if (m.shift_offset == 0 || m.shift_offset >= (1u << m.block_size)) throw Error(Error::InputValidation, "shift indicator: shift_offset must be in 1 .. 2^block_size - 1");
				if ((uint32_t)m.variant > 2) throw Error(Error::InputValidation, "shift indicator: unknown variant");
				break;
			case EvalcheckMultilinear::TowerBasis:
				if (m.k != p.n_vars || m.iota + m.k > 7) throw Error(Error::InputValidation, "tower basis: k must equal the prover's number of variables and iota + k <= 7");
				break;
			default: throw Error(Error::InputValidation, "unknown multilinear kind");
			}
		}
		total_m += p.multilins.size();
	}
	if (provers.empty()) return {};
	if (scratch.len_ < evalcheck_scratch_elems(provers)) throw Error(Error::InputValidation, "scratch holds fewer than evalcheck_scratch_elems elements");
	DeviceBumpAllocator alloc(scratch);

	// ---- collect_projected_mles: distinct suffixes expanded once, all projections of a suffix in one call, duplicates once
	// (a linear combination is projected from its constituents by the op that XORs them on load; the whole term list travels with
	// every call, a job names its range)
	struct SuffixJob {
		FSlice query;
		std::vector<bn_pe_column> cols;
		std::vector<void *> outs;
		std::vector<bn_pel_job> lc_jobs;
		std::vector<void *> lc_outs;
	};
	std::map<EvalcheckSuffix, SuffixJob> jobs;
	std::map<EvalcheckProjection, FSlice> projected;
	std::map<EvalcheckLinComb, FSlice> combined;
	for (const EvalcheckProver &p : provers) {
		for (const EvalcheckMultilinear &m : p.multilins) {
			if (m.kind != EvalcheckMultilinear::Projection && m.kind != EvalcheckMultilinear::LinComb) continue;
			const EvalcheckSuffix s{m.suffix_off, m.suffix_len};
			auto job = jobs.find(s);
			if (job == jobs.end()) {
				const FSliceMut q = ops::eq_ind_partial_eval(hal, alloc, std::vector<B128>(pool.begin() + m.suffix_off, pool.begin() + m.suffix_off + m.suffix_len));
				job = jobs.emplace(s, SuffixJob{ComputeMemory::as_const(q), {}, {}, {}, {}}).first;
			}
			if (m.kind == EvalcheckMultilinear::LinComb) {
				const auto lc_key = evalcheck_lincomb_key(m);
				if (combined.count(lc_key)) continue;
				FSliceMut o = alloc.alloc((size_t)1 << p.n_vars);
				job->second.lc_jobs.push_back(bn_pel_job{m.n_vars, m.first_term, m.n_terms, 0, m.offset.raw()});
				job->second.lc_outs.push_back(o.ptr);
				combined.emplace(lc_key, ComputeMemory::as_const(o));
				continue;
			}
			const auto key = evalcheck_projection_key(m);
			if (projected.count(key)) continue;
			FSliceMut o = alloc.alloc((size_t)1 << p.n_vars);
			job->second.cols.push_back(bn_pe_column{m.d_column, m.tower_level, m.n_vars});
			job->second.outs.push_back(o.ptr);
			projected.emplace(key, ComputeMemory::as_const(o));
		}
	}
	std::vector<bn_pel_term> raw_terms;
	for (const EvalcheckTerm &t : terms) raw_terms.push_back(bn_pel_term{t.d_column, t.tower_level, 0, t.coeff.raw()});
	for (auto &kv : jobs) {
		if (!kv.second.cols.empty())
			check(bn_partial_eval_high_batch(hal.raw_ctx(), kv.second.cols.data(), (uint32_t)kv.second.cols.size(), kv.second.query.ptr, kv.first.second, kv.second.outs.data()));
		if (!kv.second.lc_jobs.empty())
			check(bn_partial_eval_high_lincomb_batch(hal.raw_ctx(), kv.second.lc_jobs.data(), (uint32_t)kv.second.lc_jobs.size(), raw_terms.data(), (uint32_t)raw_terms.size(),
			                                         kv.second.query.ptr, kv.first.second, kv.second.lc_outs.data()));
	}

	// ---- the transparent tables and the provers
	std::vector<B128> host_mem(total_m + 8);
	HostBumpAllocator host_alloc(HostSliceMut{host_mem.data(), host_mem.size()});
	std::vector<std::unique_ptr<BivariateSumcheckProver>> sc;
	for (const EvalcheckProver &p : provers) {
		std::vector<FSlice> mls;
		for (const EvalcheckMultilinear &m : p.multilins) {
			if (m.kind == EvalcheckMultilinear::Projection) {
				mls.push_back(projected.at(evalcheck_projection_key(m)));
				continue;
			}
			if (m.kind == EvalcheckMultilinear::LinComb) {
				mls.push_back(combined.at(evalcheck_lincomb_key(m)));
				continue;
			}
			std::vector<B128> table;
			if (m.kind == EvalcheckMultilinear::ShiftInd) {
				table = evalcheck_shift_ind_table(m.block_size, m.shift_offset, m.variant, pool.data() + m.r_off);
			} else {
				// TowerField::basis(iota, i): ONE in limb i of 2^iota bits (tower_basis.rs:54-70)
				for (size_t i = 0; i < ((size_t)1 << m.k); i++) {
					const size_t bit = i << m.iota;
					table.push_back(bit < 64 ? B128((uint64_t)1 << bit, 0) : B128(0, (uint64_t)1 << (bit - 64)));
				}
			}
			FSliceMut d = alloc.alloc(table.size());
			hal.copy_h2d(table, d);
			mls.push_back(ComputeMemory::as_const(d));
		}
		for (const IndexCompositionBivariate &c : p.compositions)
			if (c.indices[0] >= p.multilins.size() || c.indices[1] >= p.multilins.size()) throw Error(Error::InputValidation, "a claim's index leaves its prover's multilinears");
		sc.push_back(std::make_unique<BivariateSumcheckProver>(hal, alloc, host_alloc, p.n_vars, p.compositions, p.sums, mls));
	}
	const std::vector<B128> batch_coeffs = tr.sample_vec(EvalcheckBatchCoeffs, 0, sc.size());
	return SumcheckBatchProver<BivariateSumcheckProver>(std::move(sc), batch_coeffs).run(tr, EvalcheckChallenges);
}
inline EvalcheckOutput evalcheck_bivariate_prove(ComputeLayer &hal, const std::vector<EvalcheckProver> &provers, const std::vector<B128> &pool, FSliceMut scratch,
                                                 const std::vector<B128> &batch_coeffs, const std::vector<B128> &challenges,
                                                 const std::vector<EvalcheckTerm> &terms = {})
{
	if (batch_coeffs.size() != provers.size()) throw Error(Error::InputValidation, "IncorrectNumberOfBatchCoeffs");
	if (!provers.empty() && challenges.size() < provers.back().n_vars) throw Error(Error::InputValidation, "too few challenges");
	ArrayTranscript tr({ArrayTranscript::stream(batch_coeffs), ArrayTranscript::stream(challenges)});
	return evalcheck_bivariate_prove(hal, provers, pool, scratch, tr, terms);
}

// ---- the evaluations in front of a round (prove.rs:191-275)
struct EvalcheckEvalClaim {
	const void *d_column = nullptr; // 2^n_vars values of tower_level, packed into F, only read
	uint32_t tower_level = 0, n_vars = 0;
	uint32_t point_off = 0, point_len = 0; // the point pool[point_off .. + point_len), point_len == n_vars
};

// The low part of every point has min(|point| / 2, kEvalcheckLoSplit) coordinates (<= BN_ME_MAX_LO_VARS).  Measured at 256 B1 columns
// of 2^22 bits (profiles/r15/README.md): the sweep over 6, 8, 10.
constexpr uint32_t kEvalcheckLoSplit = 8;
inline uint32_t evalcheck_lo_vars(uint32_t point_len, uint32_t lo_split = kEvalcheckLoSplit) { return std::min(point_len / 2, lo_split); }

// Exact: 2^len per distinct prefix slice and per distinct suffix slice of the pool.
inline size_t evalcheck_evaluate_scratch_elems(const std::vector<EvalcheckEvalClaim> &claims, uint32_t lo_split = kEvalcheckLoSplit)
{
	if (lo_split > BN_ME_MAX_LO_VARS) throw Error(Error::InputValidation, "the split of a point is at most BN_ME_MAX_LO_VARS");
	std::map<EvalcheckSuffix, bool> prefixes, suffixes;
	size_t total = 0;
	for (const EvalcheckEvalClaim &c : claims) {
		if (c.point_len > BN_PE_MAX_VARS) throw Error(Error::InputValidation, "a point has at most BN_PE_MAX_VARS coordinates");
		const uint32_t lo = evalcheck_lo_vars(c.point_len, lo_split);
		if (prefixes.emplace(EvalcheckSuffix{c.point_off, lo}, true).second) total += (size_t)1 << lo;
		if (suffixes.emplace(EvalcheckSuffix{c.point_off + lo, c.point_len - lo}, true).second) total += (size_t)1 << (c.point_len - lo);
	}
	return total;
}

struct EvalcheckEvaluateOutput {
	std::vector<B128> evals; // in claim order
	enum { Expand = 0, Evaluate = 1, NPhases = 2 };
	double phase_ms[NPhases] = {};
};

// Every distinct prefix and suffix slice is expanded once (memoize_query_par, subclaims.rs:489-508), a repeated (column, level, point)
// is evaluated once (visited_claims), and ONE bn_mle_evaluate_batch serves everything.
inline EvalcheckEvaluateOutput evalcheck_evaluate_claims(ComputeLayer &hal, const std::vector<EvalcheckEvalClaim> &claims, const std::vector<B128> &pool, FSliceMut scratch)
{
	for (const EvalcheckEvalClaim &c : claims) {
		if (!c.d_column) throw Error(Error::InputValidation, "null column");
		if (c.tower_level > 7 || c.tower_level == 1 || c.tower_level == 2) throw Error(Error::InputValidation, "unsupported value of tower_level");
		if (c.point_len != c.n_vars) throw Error(Error::InputValidation, "a claim's point has n_vars coordinates");
		if ((size_t)c.point_off + c.point_len > pool.size()) throw Error(Error::InputValidation, "a point leaves the point pool");
	}
	if (scratch.len_ < evalcheck_evaluate_scratch_elems(claims)) throw Error(Error::InputValidation, "scratch holds fewer than evalcheck_evaluate_scratch_elems elements");
	EvalcheckEvaluateOutput out;
	out.evals.assign(claims.size(), B128::ZERO());
	if (claims.empty()) return out;
	const auto t_begin = std::chrono::steady_clock::now();
	DeviceBumpAllocator alloc(scratch);
	std::map<EvalcheckSuffix, const void *> prefixes, suffixes;
	auto table = [&](std::map<EvalcheckSuffix, const void *> &memo, uint32_t off, uint32_t len) {
		auto it = memo.find({off, len});
		if (it == memo.end()) {
			const FSliceMut t = ops::eq_ind_partial_eval(hal, alloc, std::vector<B128>(pool.begin() + off, pool.begin() + off + len), /*expand_empty=*/false);
			it = memo.emplace(EvalcheckSuffix{off, len}, t.ptr).first;
		}
		return it->second;
	};
	std::map<EvalcheckSuffix, uint32_t> point_index;
	std::vector<bn_me_point> points;
	using ClaimKey = std::pair<std::pair<const void *, uint32_t>, EvalcheckSuffix>; // (column, level), point
	std::map<ClaimKey, uint32_t> visited;
	std::vector<bn_me_job> jobs;
	std::vector<uint32_t> job_of(claims.size());
	for (size_t i = 0; i < claims.size(); i++) {
		const EvalcheckEvalClaim &c = claims[i];
		const ClaimKey key{{c.d_column, c.tower_level}, {c.point_off, c.point_len}};
		auto seen = visited.find(key);
		if (seen == visited.end()) {
			auto pt = point_index.find({c.point_off, c.point_len});
			if (pt == point_index.end()) {
				const uint32_t lo = evalcheck_lo_vars(c.point_len);
				const void *d_lo = table(prefixes, c.point_off, lo), *d_hi = table(suffixes, c.point_off + lo, c.point_len - lo);
				pt = point_index.emplace(EvalcheckSuffix{c.point_off, c.point_len}, (uint32_t)points.size()).first;
				points.push_back(bn_me_point{d_lo, d_hi, lo, c.point_len - lo});
			}
			seen = visited.emplace(key, (uint32_t)jobs.size()).first;
			jobs.push_back(bn_me_job{c.d_column, c.tower_level, c.n_vars, pt->second, 0});
		}
		job_of[i] = seen->second;
	}
	const auto t_expand = std::chrono::steady_clock::now();
	out.phase_ms[EvalcheckEvaluateOutput::Expand] = elapsed_ms(t_begin, t_expand);
	std::vector<bn_f128> vals(jobs.size());
	check(bn_mle_evaluate_batch(hal.raw_ctx(), jobs.data(), (uint32_t)jobs.size(), points.data(), (uint32_t)points.size(), vals.data()));
	for (size_t i = 0; i < claims.size(); i++) out.evals[i] = B128(vals[job_of[i]].lo, vals[job_of[i]].hi);
	out.phase_ms[EvalcheckEvaluateOutput::Evaluate] = elapsed_ms(t_expand);
	return out;
}

} // namespace binius_amd
