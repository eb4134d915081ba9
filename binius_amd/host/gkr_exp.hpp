// binius_amd/host/gkr_exp.hpp -- C++ mirror of the GKR exponentiation argument's batch prover, gkr_exp::batch_prove
// (crates/core/src/protocols/gkr_exp/batch_prove.rs:46-315), which the constraint system runs for every Exp its tables declare
// (core/src/constraint_system/prove.rs:186-195 the witness, :236-274 the prover, EvaluationOrder::HighToLow):
//
//   BaseExpWitness::new_with_*_base        witness.rs:31-110, 139-156, 258-284   ONE call of bn_exp_circuit_layers for all witnesses
//   claims sorted by n_vars, descending    batch_prove.rs:73-76                  else ClaimsOutOfOrder; :63-65 MismatchedWitnessClaimLength
//   build_layer_gkr_sumcheck_provers       batch_prove.rs:123-196                consecutive provers with equal evaluation points form a
//                                                                                group: ONE EqIndPointProver (eq_ind.hpp; the
//                                                                                reference builds it from the same, common.rs:110-113) over
//                                                                                the concatenated multilinears, one composition per prover
//   layer_composite_sum_claim              provers.rs:117-165, 256-312           static, not last:  [V_{w-2-L}, e_{w-1-L}]      x0 ((1 - x1) + x1 c), c = g^(2^(w-1-L))
//     compositions.rs:43-61                                                      static, last:      nothing (no claim, no multilinears)
//                                                                                dynamic, not last: [V_{w-2-L}, e_L, base]      x0^2 ((1 - x1) + x1 x2), degree 4
//                                                                                dynamic, last:     [base, e_{w-1}]             (1 - x1) + x1 x0
//   sumcheck::batch_prove                  prove/batch_sumcheck.rs:102-199       SumcheckBatchProver, JoinBySize (batch_prover.hpp):
//                                                                                provers by n_vars descending; a prover's batch coefficient is
//                                                                                taken when the round with its n_vars begins; round proof =
//                                                                                sum of coefficient x its round coefficients, padded to the
//                                                                                longest, last coefficient dropped; finish() of every prover
//                                                                                (the indicator's evaluation last); challenges reversed
//   build_layer_exponent_bit_claims        batch_prove.rs:254-291                the indicator evaluations dropped, every prover handed its own
//   finish_layer                           provers.rs:171-218, 318-370           point = r[..n_vars]; the claim moves to the input layer's
//     first_layer_inverse                  utils.rs:5-10                         evaluation; LayerClaims: the bit, then (dynamic) the base;
//                                                                                static last layer: (eval - 1) (g - 1)^-1 at the current point
//   provers.retain                         batch_prove.rs:112
//
// A group of zero variables has no rounds: its "final evaluations" are the single elements of its multilinears and the indicator's
// prefix is ONE (EqIndPointProver's zero-variable case).
// Memory: the sumcheck folds in place and a layer V_k is a multilinear of exactly one sumcheck, so the arenas are CONSUMED.  Before a
// layer's sumcheck its bit columns are expanded into the scratch as B128 multilinears (bn_bits_to_b128, one launch for all), and the
// base column of every active dynamic prover is copied there: the caller owns it and every layer needs it again.  The scratch is
// reused layer by layer; gkr_exp_scratch_elems is the exact requirement.  The reference's immediate_switchover_heuristic folds at once
// too; a B1-transparent route would not change the transcript.
//
// Transcript samples, fixed stride so that a caller need not predict the grouping: batch_coeffs[L * n_claims + g] is the coefficient
// of the g-th sumcheck prover of layer L (g counts the groups that yield a prover, in order; unused slots are ignored),
// challenges[L * max_n_vars + r] the challenge of round r of layer L.
//
// Protocol bookkeeping only: every hypercube-sized operation is a call of the backend.
#pragma once
#include <algorithm>
#include <chrono>
#include <memory>

#include "batch_prover.hpp"
#include "eq_ind.hpp"

namespace binius_amd {

struct GkrExpClaim {
	size_t n_vars = 0, width = 0;
	bool dynamic = false;
	B128 static_base{};
	FSlice base{};                 // dynamic: 2^n_vars elements, only read
	std::vector<const void *> bits; // width packed bit columns, e_0 first, only read
	FSliceMut arena{};             // width * 2^n_vars elements: filled here, then consumed
	std::vector<B128> eval_point;  // n_vars coordinates
	B128 eval{};
};

struct GkrExpLayerClaim {
	std::vector<B128> eval_point;
	B128 eval{};
};

struct GkrExpOutput {
	std::vector<std::vector<std::vector<B128>>> round_proofs;   // [layer][round]: the coefficients written to the transcript
	std::vector<std::vector<std::vector<B128>>> multilinear_evals; // [layer][sumcheck prover]: its evaluations, the indicator's last
	std::vector<std::vector<GkrExpLayerClaim>> layer_claims;    // [layer]: per prover the bit claim, then (dynamic) the base claim
	std::vector<double> layer_ms;
};

// Per claim: one column for the expanded bit column, one more for the copy of a dynamic base, and half a column for the table of the
// indicator (every claim may be a group of its own); nothing for the table at n_vars = 0.
inline size_t gkr_exp_scratch_elems(const std::vector<size_t> &n_vars, const std::vector<bool> &dynamic)
{
	size_t total = 0;
	for (size_t t = 0; t < n_vars.size(); t++)
		total += ((size_t)(dynamic[t] ? 2 : 1) << n_vars[t]) + (n_vars[t] >= 1 ? (size_t)1 << (n_vars[t] - 1) : 0);
	return total;
}

// The transcript's streams, as the array form names them: batch_coeffs[L * n_claims + g], the coefficient of the g-th sumcheck prover of
// layer L; challenges[L * max_n_vars + r], round r of layer L.
// Schedule of layer L (sumcheck::batch_prove, batch_sumcheck.rs:138-187): per round, first one batch coefficient for every prover that
// joins in it, then write the truncated round polynomial, sample 1; after the last round one coefficient per zero-variable prover;
// then every prover's evaluations are written, in order.  A layer without a prover writes and draws nothing.
enum { GkrExpBatchCoeffs = 0, GkrExpChallenges = 1 };
inline GkrExpOutput gkr_exp_batch_prove(ComputeLayer &hal, Mi355xBackend &backend, size_t n_witnesses, const std::vector<GkrExpClaim> &claims, FSliceMut scratch,
                                        TranscriptSource &tr)
{
	const size_t k = claims.size();
	if (n_witnesses != k) throw Error(Error::InputValidation, "MismatchedWitnessClaimLength");
	GkrExpOutput out;
	if (k == 0) return out;
	size_t max_w = 0, max_n = 0;
	std::vector<size_t> nv(k);
	std::vector<bool> dyn(k);
	for (size_t t = 0; t < k; t++) {
		const GkrExpClaim &c = claims[t];
		if (t && c.n_vars > claims[t - 1].n_vars) throw Error(Error::InputValidation, "ClaimsOutOfOrder");
		if (c.eval_point.size() != c.n_vars) throw Error(Error::InputValidation, "an evaluation point has n_vars coordinates");
		if (c.bits.size() != c.width) throw Error(Error::InputValidation, "one bit column per exponent bit");
		max_w = std::max(max_w, c.width);
		max_n = std::max(max_n, c.n_vars);
		nv[t] = c.n_vars;
		dyn[t] = c.dynamic;
	}
	if (scratch.len_ < gkr_exp_scratch_elems(nv, dyn)) throw Error(Error::InputValidation, "scratch holds fewer than gkr_exp_scratch_elems elements");

	// ---- the witnesses: every layer of every circuit in one call (which validates widths, n_vars, pointers and overlaps)
	{
		std::vector<uint32_t> n32(k), w32(k), kinds(k);
		std::vector<const void *> cols, bases(k);
		std::vector<bn_f128> sb(k);
		std::vector<void *> ars(k);
		for (size_t t = 0; t < k; t++) {
			const GkrExpClaim &c = claims[t];
			if (c.width >= 1 && c.width <= BN_EXP_MAX_WIDTH && c.n_vars <= BN_EXP_MAX_VARS && c.arena.len_ != c.width << c.n_vars)
				throw Error(Error::InputValidation, "an arena holds width * 2^n_vars elements");
			n32[t] = (uint32_t)c.n_vars;
			w32[t] = (uint32_t)c.width;
			kinds[t] = c.dynamic ? BN_EXP_DYNAMIC : BN_EXP_STATIC;
			cols.insert(cols.end(), c.bits.begin(), c.bits.end());
			sb[t] = c.static_base.raw();
			bases[t] = c.base.ptr;
			ars[t] = c.arena.ptr;
		}
		if (cols.empty()) cols.push_back(nullptr);
		check(bn_exp_circuit_layers(hal.raw_ctx(), (uint32_t)k, n32.data(), w32.data(), kinds.data(), cols.data(), sb.data(), bases.data(), ars.data()));
	}

	struct Prover {
		size_t t;
		std::vector<B128> point;
		B128 eval;
	};
	std::vector<Prover> provers;
	for (size_t t = 0; t < k; t++) provers.push_back(Prover{t, claims[t].eval_point, claims[t].eval});
	auto is_last = [&](const Prover &p, size_t L) { return claims[p.t].width - 1 - L == 0; };
	auto n_mls = [&](const Prover &p, size_t L) -> size_t { return claims[p.t].dynamic ? (is_last(p, L) ? 2 : 3) : (is_last(p, L) ? 0 : 2); };
	const ArithCircuit one = ArithCircuit::constant(B128::ONE());

	for (size_t L = 0; L < max_w; L++) {
		const auto t_begin = std::chrono::steady_clock::now();
		DeviceBumpAllocator alloc(scratch);
		// ---- this layer's bit columns as B128 multilinears, the dynamic bases' copies
		std::vector<FSlice> bit_ml(provers.size()), base_ml(provers.size());
		{
			std::vector<uint32_t> ll;
			std::vector<const void *> srcs;
			std::vector<void *> dsts;
			for (size_t i = 0; i < provers.size(); i++) {
				const GkrExpClaim &c = claims[provers[i].t];
				if (n_mls(provers[i], L) == 0) continue;
				const size_t rows = (size_t)1 << c.n_vars;
				FSliceMut b = alloc.alloc(rows);
				ll.push_back((uint32_t)c.n_vars);
				srcs.push_back(c.bits[c.dynamic ? L : c.width - 1 - L]);
				dsts.push_back(b.ptr);
				bit_ml[i] = ComputeMemory::as_const(b);
				if (c.dynamic) {
					FSliceMut copy = alloc.alloc(rows);
					hal.copy_d2d(c.base, copy);
					base_ml[i] = ComputeMemory::as_const(copy);
				}
			}
			check(bn_bits_to_b128(hal.raw_ctx(), (uint32_t)ll.size(), ll.data(), srcs.data(), dsts.data()));
		}
		// ---- groups of consecutive provers with equal points; one sumcheck prover per group that has a claim
		std::vector<std::unique_ptr<EqIndPointProver>> groups;
		for (size_t i0 = 0; i0 < provers.size();) {
			size_t i1 = i0 + 1;
			while (i1 < provers.size() && provers[i1].point == provers[i0].point) i1++;
			std::vector<FSlice> mls;
			std::vector<EqIndComposition> comps;
			std::vector<B128> sums;
			for (size_t i = i0; i < i1; i++) {
				const Prover &p = provers[i];
				const GkrExpClaim &c = claims[p.t];
				const size_t rows = (size_t)1 << c.n_vars, at = mls.size();
				if (n_mls(p, L) == 0) continue;
				const ArithCircuit x0 = ArithCircuit::var(at), x1 = ArithCircuit::var(at + 1), x2 = ArithCircuit::var(at + 2);
				EqIndComposition ec;
				if (is_last(p, L)) { // (dynamic)
					mls.push_back(base_ml[i]);
					mls.push_back(bit_ml[i]);
					ec.composition = hal.compile_expr((one + x1) + x1 * x0);
					ec.composition_at_infinity = hal.compile_expr(x1 * x0);
					ec.degree = 2;
				} else {
					mls.push_back(FSlice{(const char *)c.arena.ptr + (c.width - 2 - L) * rows * sizeof(B128), rows});
					mls.push_back(bit_ml[i]);
					if (c.dynamic) {
						mls.push_back(base_ml[i]);
						ec.composition = hal.compile_expr(x0.pow(2) * ((one + x1) + x1 * x2));
						ec.composition_at_infinity = hal.compile_expr(x0.pow(2) * (x1 * x2));
						ec.degree = 4;
					} else {
						B128 power = c.static_base;
						for (size_t s = 0; s < c.width - 1 - L; s++) power = power * power;
						ec.composition = hal.compile_expr(x0 * ((one + x1) + x1 * ArithCircuit::constant(power)));
						ec.composition_at_infinity = hal.compile_expr((x0 * x1) * ArithCircuit::constant(power + B128::ONE()));
						ec.degree = 2;
					}
				}
				comps.push_back(ec);
				sums.push_back(p.eval);
			}
			if (!comps.empty())
				groups.push_back(std::make_unique<EqIndPointProver>(hal, backend, alloc, provers[i0].point.size(), std::move(mls), std::move(comps), std::move(sums), provers[i0].point));
			i0 = i1;
		}
		// ---- sumcheck::batch_prove: the groups descend by n_vars and join as the rounds reach their size
		const size_t n_groups = groups.size();
		BatchSumcheckOutput res = SumcheckBatchProver<EqIndPointProver>(std::move(groups), std::vector<B128>(n_groups), BatchSchedule::JoinBySize)
		                              .run(tr, GkrExpChallenges, L * max_n, GkrExpBatchCoeffs, L * k);
		const std::vector<B128> r(res.challenges.rbegin(), res.challenges.rend()); // reversed
		const std::vector<std::vector<B128>> &evals = res.multilinear_evals;
		// ---- build_layer_exponent_bit_claims
		std::vector<B128> flat;
		for (const auto &e : evals) flat.insert(flat.end(), e.begin(), e.end() - 1);
		std::vector<GkrExpLayerClaim> layer_claims;
		size_t at = 0;
		for (Prover &p : provers) {
			const GkrExpClaim &c = claims[p.t];
			const size_t m = n_mls(p, L);
			if (m == 0) {
				layer_claims.push_back(GkrExpLayerClaim{p.point, (p.eval + B128::ONE()) * (c.static_base + B128::ONE()).invert_or_zero()});
				continue;
			}
			const std::vector<B128> point(r.begin(), r.begin() + p.point.size());
			layer_claims.push_back(GkrExpLayerClaim{point, flat[at + 1]});
			if (c.dynamic) layer_claims.push_back(GkrExpLayerClaim{point, is_last(p, L) ? flat[at] : flat[at + 2]});
			if (!is_last(p, L)) {
				p.point = point;
				p.eval = flat[at];
			}
			at += m;
		}
		out.round_proofs.push_back(std::move(res.round_proofs));
		out.multilinear_evals.push_back(std::move(res.multilinear_evals));
		out.layer_claims.push_back(std::move(layer_claims));
		provers.erase(std::remove_if(provers.begin(), provers.end(), [&](const Prover &p) { return is_last(p, L); }), provers.end());
		out.layer_ms.push_back(elapsed_ms(t_begin));
	}
	return out;
}
inline GkrExpOutput gkr_exp_batch_prove(ComputeLayer &hal, Mi355xBackend &backend, size_t n_witnesses, const std::vector<GkrExpClaim> &claims, FSliceMut scratch,
                                        const std::vector<B128> &batch_coeffs, const std::vector<B128> &challenges)
{
	size_t max_w = 0, max_n = 0;
	for (const GkrExpClaim &c : claims) {
		max_w = std::max(max_w, c.width);
		max_n = std::max(max_n, c.n_vars);
	}
	if (n_witnesses == claims.size() && (batch_coeffs.size() < max_w * claims.size() || challenges.size() < max_w * max_n))
		throw Error(Error::InputValidation, "too few transcript samples (max_width x n_claims, max_width x max_n_vars)");
	ArrayTranscript tr({ArrayTranscript::stream(batch_coeffs), ArrayTranscript::stream(challenges)});
	return gkr_exp_batch_prove(hal, backend, n_witnesses, claims, scratch, tr);
}

} // namespace binius_amd
