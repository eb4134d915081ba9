// binius_amd/host/flush.hpp -- C++ mirror of the product-check phase of the constraint-system prover
// (crates/core/src/constraint_system/prove.rs:276-428): the grand-product argument over every flush and non-zero oracle, with the
// flush witnesses made on the device and the claims on the composite flush oracles reduced to claims on their inner columns.
//
//   mixing powers by entry position     prove.rs:744-771      const_term = r_channel + sum_const base alpha^k; an Oracle entry's
//                                                             coefficient is its alpha^k (constants take a power too)
//   make_masked_flush_witnesses         prove.rs:671-881      ONE bn_flush_witness_batch for all flushes; the witnesses stay on the
//                                                             device, truncated to the selectors' prefix (count_zero_suffixes, :883-902)
//   convert_witnesses_to_fast_ext       prove.rs:291-292      the non-zero columns widened to B128: ONE bn_partial_eval_high_batch
//                                                             at query_vars = 0 (the tower basis is kept, as in gkr_gpa.hpp)
//   Error::Zeros                        prove.rs:309-316      a zero non-zero product ends the call before anything else runs
//   gkr_gpa::batch_prove                prove.rs:386-400      gkr_gpa_batch_prove over chain(flush witnesses, non-zero witnesses)
//   reduce_flush_evalcheck_claims       prove.rs:1017-1117    a flush without selectors is a linear combination: its claim is passed
//                                                             through; the others are composite oracles 1 + S * L
//                                                             (constraint_system/verify.rs:519-571), grouped by equal evaluation
//                                                             point in order of first appearance (:1045-1073)
//   ConstraintSetBuilder::build_one     constraint.rs:114-129 (oracle) per group the multilinears are the sorted, de-duplicated union
//                                                             of the oracle ids, the compositions' variables remapped to it
//   prove_mlecheck_with_switchover      evalcheck/subclaims.rs:589-633   one EqIndPointProver (eq_ind.hpp) at the claims' point as a
//                                                             front-loaded batch of one (batch_prover.hpp: truncated round
//                                                             polynomials, as in gkr_gpa.hpp); challenges reversed; the indicator's evaluation is
//                                                             written with the others and dropped from the claims (:619-630)
//
// The order the reference fixes -- the non-zero products and their zero check come before the flushes -- is kept: the non-zero
// trees are built once for that check (one bn_product_tree_layers) and again, with the flushes', inside gkr_gpa_batch_prove, which
// this file calls as it is.
// Limits inherited from what it calls: n_selectors <= 7 (the composition's degree n_selectors + 1 <= kEqIndMaxDegree); one
// composite flush reads at most 16 distinct multilinears and its composition has at most 64 steps (bn_hal_round_evals).
//
// Protocol bookkeeping only: every hypercube-sized operation is a call of the backend.  The caller's columns are never written.
#pragma once
#include <algorithm>
#include <chrono>

#include "gkr_gpa.hpp"

namespace binius_amd {

struct FlushEntry {
	bool is_const = false;
	size_t id = 0;              // Oracle: the caller's oracle id
	const void *column = nullptr; // Oracle: 2^n_vars values of `level` packed into F (device, only read)
	uint32_t level = 0;
	B128 base{};                // Const
};
struct FlushSelector {
	size_t id = 0;
	const void *column = nullptr; // a packed B1 column
};
struct FlushSpec {
	size_t channel = 0, n_vars = 0;
	std::vector<FlushSelector> selectors;
	std::vector<FlushEntry> entries;
};
struct NonZeroSpec {
	size_t id = 0, n_vars = 0;
	const void *column = nullptr;
	uint32_t level = 0;
};
struct FlushMleCheck {
	size_t n_vars = 0;
	std::vector<size_t> flushes;                 // the composite flushes of the group, in order: one composition each
	std::vector<size_t> ids;                     // the group's multilinears: sorted, de-duplicated
	std::vector<std::vector<B128>> round_proofs; // per round: max(2, largest degree) + 1 coefficients
	std::vector<B128> final_evals;               // per multilinear, then the indicator's
	std::vector<B128> point;                     // the reversed challenges: the new claims are (ids[i], point, final_evals[i])
};
struct FlushProdcheckOutput {
	std::vector<uint64_t> prefix_lens; // per flush
	GkrGpaOutput gpa;                  // over chain(flushes, non-zero oracles); products: the flushes', then the non-zero ones
	std::vector<FlushMleCheck> checks;
	std::vector<size_t> linear_flushes; // flushes without selectors: their claims (gpa.final_points / final_evals) pass through
	double phase_ms[4] = {0, 0, 0, 0};  // witnesses (flush + widening + zero check), grand-product argument, reductions, total
};

// the multilinears of a composite flush in the reference's order: selectors, then the Oracle entries
inline std::vector<size_t> flush_oracle_ids(const FlushSpec &f)
{
	std::vector<size_t> ids;
	for (const FlushSelector &s : f.selectors) ids.push_back(s.id);
	for (const FlushEntry &e : f.entries)
		if (!e.is_const) ids.push_back(e.id);
	return ids;
}

// the groups of reduce_flush_evalcheck_claims as far as sizes go: flushes of equal n_vars leave the grand-product argument with the
// same point.  Per group (n_vars, flushes in order, sorted de-duplicated ids)
inline std::vector<FlushMleCheck> flush_groups(const std::vector<FlushSpec> &flushes)
{
	std::vector<FlushMleCheck> groups;
	for (size_t f = 0; f < flushes.size(); f++) {
		if (flushes[f].selectors.empty()) continue;
		size_t g = 0;
		while (g < groups.size() && groups[g].n_vars != flushes[f].n_vars) g++;
		if (g == groups.size()) {
			groups.emplace_back();
			groups[g].n_vars = flushes[f].n_vars;
		}
		groups[g].flushes.push_back(f);
		const std::vector<size_t> ids = flush_oracle_ids(flushes[f]);
		groups[g].ids.insert(groups[g].ids.end(), ids.begin(), ids.end());
	}
	for (FlushMleCheck &g : groups) {
		std::sort(g.ids.begin(), g.ids.end());
		g.ids.erase(std::unique(g.ids.begin(), g.ids.end()), g.ids.end());
	}
	return groups;
}

// One element (the query of the widening), the witnesses (2^n_vars per flush and non-zero oracle), their arenas (2^n_vars each for
// n_vars >= 1), the grand-product prover's own scratch, and the largest reduction: m 2^n + 2^(n - 1) for m multilinears of n variables.
inline size_t flush_prodcheck_scratch_elems(const std::vector<FlushSpec> &flushes, const std::vector<NonZeroSpec> &nonzero)
{
	std::vector<size_t> nv;
	for (const FlushSpec &f : flushes) nv.push_back(f.n_vars);
	for (const NonZeroSpec &z : nonzero) nv.push_back(z.n_vars);
	size_t total = 1;
	for (size_t n : nv) total += ((size_t)1 << n) + (n >= 1 ? (size_t)1 << n : 0);
	total += gkr_gpa_scratch_elems(nv);
	size_t red = 0;
	for (const FlushMleCheck &g : flush_groups(flushes)) red = std::max(red, (g.ids.size() << g.n_vars) + (g.n_vars >= 1 ? (size_t)1 << (g.n_vars - 1) : 0));
	return total + red;
}

namespace flush_detail {

struct Widen {
	const void *src;
	uint32_t level;
	size_t n_vars;
	void *dst; // 2^n_vars B128 elements
};

// Columns of any level and size as B128 multilinears: ONE bn_partial_eval_high_batch at query_vars = 0 for the columns that fill a
// 16-byte element, bn_bits_to_b128 for `bits` (selectors) and for smaller bit columns, and for smaller columns of the other levels
// the flush kernel as a copy (one column, coefficient ONE, no constant, no selector).
inline void widen(ComputeLayer &hal, const std::vector<Widen> &cols, const std::vector<Widen> &bits, const void *d_one)
{
	std::vector<bn_pe_column> pe;
	std::vector<void *> pe_out;
	std::vector<uint32_t> b_log, f_nv, f_ns, f_nc, f_lv;
	std::vector<const void *> b_src, f_src;
	std::vector<void *> b_dst, f_dst;
	std::vector<bn_f128> f_coeff, f_const;
	for (const Widen &w : bits) {
		b_log.push_back((uint32_t)w.n_vars);
		b_src.push_back(w.src);
		b_dst.push_back(w.dst);
	}
	for (const Widen &w : cols) {
		if (w.n_vars + w.level >= 7) {
			pe.push_back(bn_pe_column{w.src, w.level, (uint32_t)w.n_vars});
			pe_out.push_back(w.dst);
		} else if (w.level == 0) {
			b_log.push_back((uint32_t)w.n_vars);
			b_src.push_back(w.src);
			b_dst.push_back(w.dst);
		} else {
			f_nv.push_back((uint32_t)w.n_vars);
			f_ns.push_back(0);
			f_nc.push_back(1);
			f_lv.push_back(w.level);
			f_src.push_back(w.src);
			f_dst.push_back(w.dst);
			f_coeff.push_back(B128::ONE().raw());
			f_const.push_back(B128::ZERO().raw());
		}
	}
	if (!pe.empty()) check(bn_partial_eval_high_batch(hal.raw_ctx(), pe.data(), (uint32_t)pe.size(), d_one, 0, pe_out.data()));
	if (!b_log.empty()) check(bn_bits_to_b128(hal.raw_ctx(), (uint32_t)b_log.size(), b_log.data(), b_src.data(), b_dst.data()));
	if (!f_nv.empty()) {
		std::vector<uint64_t> lens(f_nv.size());
		check(bn_flush_witness_batch(hal.raw_ctx(), (uint32_t)f_nv.size(), f_nv.data(), f_ns.data(), nullptr, f_nc.data(), f_src.data(), f_lv.data(), f_coeff.data(),
		                             f_const.data(), f_dst.data(), lens.data()));
	}
}

} // namespace flush_detail

// The transcript's streams, as the array form names them.  gpa_*: the samples gkr_gpa_batch_prove takes (its streams 0 .. 2), sized by
// the largest n_vars over flushes and non-zero oracles.  red_batch_coeffs[g], red_challenges: per MLE-check (flush_groups order) one
// batch coefficient and its n_vars challenges, concatenated.
// Schedule (constraint_system/prove.rs:309-425): write the non-zero products; sample the mixing challenge, then the n_channels
// permutation challenges; write the flush products; the grand-product argument's schedule (gkr_gpa.hpp) over chain(flushes, non-zero);
// per MLE-check a front-loaded batch of one: sample its batch coefficient, n_vars rounds of write / sample, write its evaluations.
// A system without flushes and without non-zero oracles still writes its (empty) product slices and draws the mixing challenge and
// the n_channels permutation challenges (prove.rs:318-330 has no other case): against a caller's transcript the two draws are made
// and dropped, so that the challenger stays in step with the verifier's.  The array form, which has nothing to keep in step, returns
// at once.
enum { FlushRedBatchCoeffs = 3, FlushRedChallenges = 4, FlushMixingChallenge = 5, FlushPermutationChallenges = 6 };
inline void flush_prodcheck_empty(TranscriptSource &tr, size_t n_channels)
{
	if (!tr.observes_writes()) return;
	(void)tr.sample(FlushMixingChallenge, 0);
	(void)tr.sample_vec(FlushPermutationChallenges, 0, n_channels);
}
inline FlushProdcheckOutput flush_prodcheck_prove(ComputeLayer &hal, Mi355xBackend &backend, const std::vector<FlushSpec> &flushes, const std::vector<NonZeroSpec> &nonzero,
                                                  size_t n_channels, FSliceMut scratch, TranscriptSource &tr)
{
	using namespace flush_detail;
	const auto t_begin = std::chrono::steady_clock::now();
	const size_t nf = flushes.size(), nz = nonzero.size(), k = nf + nz;
	FlushProdcheckOutput out;
	// ---- validation (what the ops below would not say in the caller's terms)
	for (const FlushSpec &f : flushes) {
		if (f.channel >= n_channels) throw Error(Error::InputValidation, "a flush names a channel without a permutation challenge");
		if (f.n_vars > BN_FLUSH_MAX_VARS) throw Error(Error::InputValidation, "n_vars out of range (0 .. 28)");
		if (f.selectors.size() + 1 > kEqIndMaxDegree) throw Error(Error::InputValidation, "more than 7 selectors: the composite's degree exceeds the sumcheck's");
		size_t n_cols = 0;
		for (const FlushEntry &e : f.entries) n_cols += !e.is_const;
		if (n_cols == 0) throw Error(Error::InputValidation, "EmptyFlushOracles");
	}
	for (const NonZeroSpec &z : nonzero)
		if (z.n_vars > BN_PRODUCT_TREE_MAX_VARS) throw Error(Error::InputValidation, "n_vars out of range (0 .. 28)");
	const std::vector<FlushMleCheck> groups = flush_groups(flushes);
	if (scratch.len_ < flush_prodcheck_scratch_elems(flushes, nonzero)) throw Error(Error::InputValidation, "scratch holds fewer than flush_prodcheck_scratch_elems elements");
	if (k == 0) {
		flush_prodcheck_empty(tr, n_channels);
		return out;
	}

	DeviceBumpAllocator alloc(scratch);
	FSliceMut d_one = alloc.alloc(1);
	hal.fill(d_one, B128::ONE());
	std::vector<size_t> nv(k);
	std::vector<FSliceMut> wit(k), arenas(k);
	for (size_t t = 0; t < k; t++) {
		nv[t] = t < nf ? flushes[t].n_vars : nonzero[t - nf].n_vars;
		wit[t] = alloc.alloc((size_t)1 << nv[t]);
	}
	for (size_t t = 0; t < k; t++)
		if (nv[t] >= 1) arenas[t] = alloc.alloc((size_t)1 << nv[t]);

	// ---- the non-zero columns as B128 witnesses; a zero product ends the call (Error::Zeros, prove.rs:309-316)
	if (nz) {
		std::vector<Widen> cols;
		for (size_t i = 0; i < nz; i++) cols.push_back(Widen{nonzero[i].column, nonzero[i].level, nonzero[i].n_vars, wit[nf + i].ptr});
		widen(hal, cols, {}, d_one.ptr);
		std::vector<uint32_t> n32(nz);
		std::vector<const void *> ins(nz);
		std::vector<uint64_t> lens(nz);
		std::vector<void *> ars(nz);
		std::vector<bn_f128> prod(nz);
		for (size_t i = 0; i < nz; i++) {
			n32[i] = (uint32_t)nonzero[i].n_vars;
			ins[i] = wit[nf + i].ptr;
			lens[i] = wit[nf + i].len_;
			ars[i] = arenas[nf + i].ptr;
		}
		check(bn_product_tree_layers(hal.raw_ctx(), (uint32_t)nz, n32.data(), ins.data(), lens.data(), ars.data(), prod.data()));
		for (size_t i = 0; i < nz; i++)
			if (prod[i].lo == 0 && prod[i].hi == 0) throw Error(Error::InputValidation, "Zeros: the product of a non-zero oracle is zero");
		tr.write(BNH_TR_MESSAGE, prod.data(), nz * sizeof(bn_f128)); // (prove.rs:318-320)
	}
	const B128 mixing_challenge = tr.sample(FlushMixingChallenge, 0);                                            // (prove.rs:329)
	const std::vector<B128> permutation_challenges = tr.sample_vec(FlushPermutationChallenges, 0, n_channels); // (prove.rs:330)

	// ---- the flush witnesses: one call for all flushes
	std::vector<B128> const_terms(nf);
	std::vector<std::vector<B128>> coeffs(nf); // per flush: the mixing powers of its Oracle entries
	if (nf) {
		std::vector<uint32_t> n32(nf), ns(nf), nc(nf), levels;
		std::vector<const void *> sels, cols;
		std::vector<bn_f128> cf, ct(nf);
		std::vector<void *> outs(nf);
		for (size_t f = 0; f < nf; f++) {
			const FlushSpec &fl = flushes[f];
			B128 power = B128::ONE(), c = permutation_challenges[fl.channel];
			for (const FlushEntry &e : fl.entries) {
				if (e.is_const) {
					c += e.base * power;
				} else {
					coeffs[f].push_back(power);
					cols.push_back(e.column);
					levels.push_back(e.level);
					cf.push_back(power.raw());
				}
				power = power * mixing_challenge;
			}
			const_terms[f] = c;
			ct[f] = c.raw();
			n32[f] = (uint32_t)fl.n_vars;
			ns[f] = (uint32_t)fl.selectors.size();
			nc[f] = (uint32_t)coeffs[f].size();
			for (const FlushSelector &s : fl.selectors) sels.push_back(s.column);
			outs[f] = wit[f].ptr;
		}
		if (sels.empty()) sels.push_back(nullptr);
		out.prefix_lens.resize(nf);
		check(bn_flush_witness_batch(hal.raw_ctx(), (uint32_t)nf, n32.data(), ns.data(), sels.data(), nc.data(), cols.data(), levels.data(), cf.data(), ct.data(),
		                             outs.data(), out.prefix_lens.data()));
	}
	out.phase_ms[0] = elapsed_ms(t_begin);

	// ---- the grand-product argument over chain(flush witnesses with their prefix lengths, non-zero witnesses)
	const auto t_gpa = std::chrono::steady_clock::now();
	{
		std::vector<FSlice> ins(k);
		for (size_t t = 0; t < k; t++) ins[t] = FSlice{wit[t].ptr, t < nf ? (size_t)out.prefix_lens[t] : wit[t].len_};
		const size_t gpa_need = gkr_gpa_scratch_elems(nv);
		out.gpa = gkr_gpa_batch_prove(hal, backend, nv, ins, arenas, alloc.alloc(gpa_need), tr,
		                              [&](const std::vector<B128> &products) { tr.write_scalars(products.data(), nf); }); // (prove.rs:378-380)
	}
	out.phase_ms[1] = elapsed_ms(t_gpa);

	// ---- reduce_flush_evalcheck_claims
	const auto t_red = std::chrono::steady_clock::now();
	for (size_t f = 0; f < nf; f++)
		if (flushes[f].selectors.empty()) out.linear_flushes.push_back(f);
	const FSliceMut red_scratch = alloc.alloc(alloc.capacity());
	const ArithCircuit one = ArithCircuit::constant(B128::ONE());
	size_t ch_at = 0;
	for (size_t g = 0; g < groups.size(); g++) {
		FlushMleCheck chk = groups[g];
		const size_t n = chk.n_vars, rows = (size_t)1 << n, m = chk.ids.size();
		const std::vector<B128> &point = out.gpa.final_points[chk.flushes[0]];
		for (size_t f : chk.flushes)
			if (out.gpa.final_points[f] != point) throw Error(Error::CoreLibError, "flushes of equal n_vars left the grand-product argument with different points");
		DeviceBumpAllocator ra(red_scratch);
		// the group's multilinears widened to B128: every id from its first occurrence
		std::vector<FSlice> mls(m);
		{
			std::vector<Widen> cols, bits;
			std::vector<bool> have(m, false);
			for (size_t f : chk.flushes) {
				auto place = [&](size_t id, const void *src, uint32_t level, bool is_bits) {
					const size_t at = std::lower_bound(chk.ids.begin(), chk.ids.end(), id) - chk.ids.begin();
					if (have[at]) return;
					have[at] = true;
					FSliceMut d = ra.alloc(rows);
					mls[at] = ComputeMemory::as_const(d);
					(is_bits ? bits : cols).push_back(Widen{src, level, n, d.ptr});
				};
				for (const FlushSelector &s : flushes[f].selectors) place(s.id, s.column, 0, true);
				for (const FlushEntry &e : flushes[f].entries)
					if (!e.is_const) place(e.id, e.column, e.level, false);
			}
			widen(hal, cols, bits, d_one.ptr);
		}
		// one composition per claim: 1 + prod selectors * (const_term + 1 + sum coeff_j x_j), variables remapped to the union
		std::vector<EqIndComposition> comps;
		std::vector<B128> sums;
		for (size_t f : chk.flushes) {
			const FlushSpec &fl = flushes[f];
			auto var = [&](size_t id) { return ArithCircuit::var(std::lower_bound(chk.ids.begin(), chk.ids.end(), id) - chk.ids.begin()); };
			ArithCircuit sel = var(fl.selectors[0].id);
			for (size_t s = 1; s < fl.selectors.size(); s++) sel = sel * var(fl.selectors[s].id);
			ArithCircuit lin = ArithCircuit::constant(const_terms[f] + B128::ONE()), lead = ArithCircuit::constant(B128::ZERO());
			size_t j = 0;
			bool first = true;
			for (const FlushEntry &e : fl.entries) {
				if (e.is_const) continue;
				const ArithCircuit term = var(e.id) * ArithCircuit::constant(coeffs[f][j++]);
				lin = lin + term;
				lead = first ? term : lead + term;
				first = false;
			}
			EqIndComposition ec;
			ec.composition = hal.compile_expr(one + sel * lin);
			ec.composition_at_infinity = hal.compile_expr(sel * lead);
			ec.degree = fl.selectors.size() + 1;
			comps.push_back(ec);
			sums.push_back(out.gpa.final_evals[f]);
		}
		// a front-loaded batch of one; at n = 0 there are no rounds (EqIndPointProver's zero-variable case)
		const B128 red_batch_coeff = tr.sample(FlushRedBatchCoeffs, g);
		BatchSumcheckOutput res = prove_batch_of_one(std::make_unique<EqIndPointProver>(hal, backend, ra, n, mls, std::move(comps), std::move(sums), point), red_batch_coeff, tr,
		                                             FlushRedChallenges, ch_at);
		chk.round_proofs = std::move(res.round_proofs);
		chk.final_evals = std::move(res.multilinear_evals[0]);
		chk.point.assign(res.challenges.rbegin(), res.challenges.rend()); // reversed (subclaims.rs:623-624)
		ch_at += n;
		out.checks.push_back(std::move(chk));
	}
	out.phase_ms[2] = elapsed_ms(t_red);
	out.phase_ms[3] = elapsed_ms(t_begin);
	return out;
}
inline FlushProdcheckOutput flush_prodcheck_prove(ComputeLayer &hal, Mi355xBackend &backend, const std::vector<FlushSpec> &flushes, const std::vector<NonZeroSpec> &nonzero,
                                                  B128 mixing_challenge, const std::vector<B128> &permutation_challenges, FSliceMut scratch,
                                                  const std::vector<B128> &gpa_batch_coeffs, const std::vector<B128> &gpa_sumcheck_challenges,
                                                  const std::vector<B128> &gpa_challenges, const std::vector<B128> &red_batch_coeffs, const std::vector<B128> &red_challenges)
{
	size_t need = 0;
	const std::vector<FlushMleCheck> groups = flush_groups(flushes);
	for (const FlushMleCheck &g : groups) need += g.n_vars;
	if (red_batch_coeffs.size() < groups.size() || red_challenges.size() < need) throw Error(Error::InputValidation, "too few transcript samples for the reductions");
	ArrayTranscript tr({ArrayTranscript::stream(gpa_batch_coeffs), ArrayTranscript::stream(gpa_sumcheck_challenges), ArrayTranscript::stream(gpa_challenges),
	                    ArrayTranscript::stream(red_batch_coeffs), ArrayTranscript::stream(red_challenges), ArrayTranscript::Stream{&mixing_challenge, 1},
	                    ArrayTranscript::stream(permutation_challenges)});
	return flush_prodcheck_prove(hal, backend, flushes, nonzero, permutation_challenges.size(), scratch, tr);
}

} // namespace binius_amd
