// binius_amd/host/gkr_gpa.hpp -- C++ mirror of the GKR grand-product argument's batch prover, gkr_gpa::batch_prove
// (crates/core/src/protocols/gkr_gpa/prove.rs:33-296), which the constraint system runs over every flush and non-zero oracle
// (core/src/constraint_system/prove.rs:285-412, EvaluationOrder::HighToLow at :394):
//
//   GrandProductWitness::new            gkr_gpa.rs:38-90    ONE call of bn_product_tree_layers for all witnesses (every layer of
//                                                           every tree, heap order); grand_product_evaluation = its products
//   stable sort by n_vars, descending   prove.rs:61-62
//   process_finished_provers            prove.rs:143-161    the states with n_vars = j leave with the current point and evaluation
//   stage_sumcheck_provers              prove.rs:208-280    one EqIndSumcheckProver (eq_ind.hpp) over j variables: multilinears
//                                                           2i, 2i + 1 = the halves of state i's layer j + 1, claim var(2i) var(2i+1)
//                                                           with sum = its layer_eval, eq_ind_challenges = the current point
//   front_loaded::BatchProver of ONE    front_loaded.rs:122-198   SumcheckBatchProver (batch_prover.hpp): round proof = the prover's
//                                                           coefficients times the batch coefficient, last coefficient dropped
//   challenges reversed, gpa_challenge  prove.rs:106-116    eval_point = reversed challenges || gpa_challenge
//   update_layer_eval                   prove.rs:282-284    layer_eval = e0 + gpa_challenge (e1 - e0)
//
// Step 0 has zero variables: no rounds, the final evaluations are the two elements of layer 1 and the indicator's prefix is ONE
// (EqIndPointProver's zero-variable case, two elements per layer).
// The sumcheck folds in place, so the arenas are consumed.  A tree's last step runs over its INPUT layer, which the caller owns and
// which may be truncated: every input is first copied into the scratch, padded with ONEs to 2^n_vars elements (bn_pad_with_ones, one
// launch for all), and the copy is folded; the inputs are never written.  The sumcheck over a truncated input just sees the ONEs
// (with_const_suffixes, prove.rs:262-264, is an optimisation of the reference's CPU path).
// Scratch: sum over the claims with n_vars >= 1 of 2^n_vars elements, plus 2^(max n_vars - 1) for the indicator's table.
//
// Protocol bookkeeping only: every hypercube-sized operation is a call of the backend.
#pragma once
#include <algorithm>
#include <chrono>

#include <functional>

#include "batch_prover.hpp"
#include "eq_ind.hpp"

namespace binius_amd {

struct GkrGpaOutput {
	std::vector<B128> products;                      // per claim, the callers' order
	std::vector<std::vector<B128>> round_proofs;     // per step j: 3 j coefficients (j rounds of 3)
	std::vector<std::vector<B128>> layer_evals;      // per step: 2 * active evaluations (sorted order), then the indicator's prefix
	std::vector<std::vector<B128>> final_points;     // per claim (LayerClaim::eval_point, n_vars coordinates), the callers' order (unsort, :140)
	std::vector<B128> final_evals;                   // per claim (LayerClaim::eval)
	std::vector<double> step_ms;                     // wall time per step
};

inline size_t gkr_gpa_scratch_elems(const std::vector<size_t> &n_vars)
{
	size_t total = 0, max_n = 0;
	for (size_t n : n_vars) {
		if (n >= 1) total += (size_t)1 << n;
		max_n = std::max(max_n, n);
	}
	return total + (max_n >= 1 ? (size_t)1 << (max_n - 1) : 0);
}

// The transcript's streams, as the array form names them: batch_coeffs[j], gpa_challenges[j]: one per step j < max n_vars (step 0's
// batch coefficient is sampled and unused); sumcheck_challenges: step j's j challenges, steps concatenated.
// Schedule of step j (prove.rs:79-126): sample the batch coefficient (front_loaded::BatchProver::new, sample_vec(1)); j rounds of
// write 3 coefficients / sample 1; write the 2 * active layer evaluations and the indicator's; sample the layer challenge.
enum { GkrGpaBatchCoeffs = 0, GkrGpaSumcheckChallenges = 1, GkrGpaChallenges = 2 };
inline GkrGpaOutput gkr_gpa_batch_prove(ComputeLayer &hal, Mi355xBackend &backend, const std::vector<size_t> &n_vars, const std::vector<FSlice> &inputs,
                                        const std::vector<FSliceMut> &arenas, FSliceMut scratch, TranscriptSource &tr,
                                        const std::function<void(const std::vector<B128> &)> &on_products = nullptr)
{
	const size_t k = n_vars.size();
	if (inputs.size() != k || arenas.size() != k) throw Error(Error::InputValidation, "MismatchedWitnessClaimLength");
	if (scratch.len_ < gkr_gpa_scratch_elems(n_vars)) throw Error(Error::InputValidation, "scratch holds fewer than sum 2^n_vars + 2^(max n_vars - 1) elements");
	GkrGpaOutput out;
	out.products.resize(k);
	out.final_points.resize(k);
	out.final_evals.resize(k);
	if (k == 0) return out;

	// ---- the witnesses: every layer of every tree in one call
	{
		std::vector<uint32_t> nv(k);
		std::vector<const void *> ins(k);
		std::vector<uint64_t> lens(k);
		std::vector<void *> ars(k);
		for (size_t t = 0; t < k; t++) {
			if (n_vars[t] >= 1 && arenas[t].len_ != (size_t)1 << n_vars[t]) throw Error(Error::InputValidation, "an arena holds 2^n_vars elements");
			nv[t] = (uint32_t)n_vars[t];
			ins[t] = inputs[t].len_ ? inputs[t].ptr : nullptr;
			lens[t] = inputs[t].len_;
			ars[t] = arenas[t].ptr;
		}
		check(bn_product_tree_layers(hal.raw_ctx(), (uint32_t)k, nv.data(), ins.data(), lens.data(), ars.data(), reinterpret_cast<bn_f128 *>(out.products.data())));
	}
	// (a caller that writes products to the transcript does it here, before the first sample of the argument)
	if (on_products) on_products(out.products);
	// ---- full-length copies of the inputs (the last layer each tree's sumchecks fold)
	std::vector<FSliceMut> padded(k);
	size_t used = 0;
	{
		std::vector<uint32_t> ll;
		std::vector<const void *> srcs;
		std::vector<uint64_t> lens;
		std::vector<void *> dsts;
		for (size_t t = 0; t < k; t++) {
			if (n_vars[t] == 0) continue;
			padded[t] = FSliceMut{(char *)scratch.ptr + used * sizeof(B128), (size_t)1 << n_vars[t]};
			used += padded[t].len_;
			ll.push_back((uint32_t)n_vars[t]);
			srcs.push_back(inputs[t].len_ ? inputs[t].ptr : nullptr);
			lens.push_back(inputs[t].len_);
			dsts.push_back(padded[t].ptr);
		}
		check(bn_pad_with_ones(hal.raw_ctx(), (uint32_t)ll.size(), ll.data(), srcs.data(), lens.data(), dsts.data()));
	}
	const FSliceMut eq_scratch{(char *)scratch.ptr + used * sizeof(B128), scratch.len_ - used};

	// ---- the states, sorted stably by n_vars descending (:61-62)
	std::vector<size_t> order(k);
	for (size_t t = 0; t < k; t++) order[t] = t;
	std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return n_vars[a] > n_vars[b]; });
	std::vector<B128> layer_eval = out.products; // (GrandProductProverState::new, :185-189)
	std::vector<B128> eval_point;
	// claim i of a step is var(2i) var(2i + 1); its leading form is itself
	std::vector<EqIndComposition> all_comps;
	size_t n_multi = 0;
	for (size_t n : n_vars) n_multi += n >= 2;
	for (size_t i = 0; i < n_multi; i++) {
		EqIndComposition ec;
		ec.composition = hal.compile_expr(ArithCircuit::var(2 * i) * ArithCircuit::var(2 * i + 1));
		ec.composition_at_infinity = ec.composition;
		ec.degree = 2;
		all_comps.push_back(ec);
	}
	size_t ch_at = 0;
	for (size_t j = 0;; j++) {
		// process_finished_provers (:143-161)
		for (size_t t : order)
			if (n_vars[t] == j) {
				out.final_points[t] = eval_point;
				out.final_evals[t] = layer_eval[t];
			}
		std::vector<size_t> active;
		for (size_t t : order)
			if (n_vars[t] > j) active.push_back(t);
		if (active.empty()) break;
		const auto t_begin = std::chrono::steady_clock::now();
		const B128 batch_coeff = tr.sample(GkrGpaBatchCoeffs, j);
		// layer j + 1 of every active state: its arena, or the padded copy of its input
		std::vector<const char *> layer(active.size());
		for (size_t i = 0; i < active.size(); i++) {
			const size_t t = active[i];
			layer[i] = j + 1 == n_vars[t] ? (const char *)padded[t].ptr : (const char *)arenas[t].ptr + (((size_t)1 << (j + 1)) * sizeof(B128));
		}
		// j >= 1: the halves of the layer are multilinears 2i, 2i + 1; j = 0: both elements of layer 1 are read in one piece
		const size_t half = (size_t)1 << j;
		std::vector<FSlice> slices;
		std::vector<B128> sums;
		for (size_t i = 0; i < active.size(); i++) {
			slices.push_back(FSlice{layer[i], j ? half : 2});
			if (j) slices.push_back(FSlice{layer[i] + half * sizeof(B128), half});
			sums.push_back(layer_eval[active[i]]);
		}
		DeviceBumpAllocator eq_alloc(eq_scratch);
		// (step 0 has no rounds and takes no composition)
		auto prover = std::make_unique<EqIndPointProver>(hal, backend, eq_alloc, j, std::move(slices), std::vector<EqIndComposition>(all_comps.begin(), all_comps.begin() + (j ? active.size() : 0)),
		                                                 std::move(sums), eval_point, j ? 1 : 2);
		BatchSumcheckOutput res = prove_batch_of_one(std::move(prover), batch_coeff, tr, GkrGpaSumcheckChallenges, ch_at);
		// (the layer challenge is drawn after the layer's evaluations are written, prove.rs:113-114)
		const B128 gpa_challenge = tr.sample(GkrGpaChallenges, j);
		std::vector<B128> proofs;
		for (const auto &rp : res.round_proofs) proofs.insert(proofs.end(), rp.begin(), rp.end());
		const std::vector<B128> finals = std::move(res.multilinear_evals[0]);
		eval_point = res.challenges;
		std::reverse(eval_point.begin(), eval_point.end()); // (:106-108)
		ch_at += j;
		eval_point.push_back(gpa_challenge);
		for (size_t i = 0; i < active.size(); i++) {
			const B128 e0 = finals[2 * i], e1 = finals[2 * i + 1];
			layer_eval[active[i]] = e0 + gpa_challenge * (e1 + e0); // extrapolate_line_scalar (:282-284)
		}
		out.round_proofs.push_back(std::move(proofs));
		out.layer_evals.push_back(finals);
		out.step_ms.push_back(elapsed_ms(t_begin));
	}
	return out;
}
inline GkrGpaOutput gkr_gpa_batch_prove(ComputeLayer &hal, Mi355xBackend &backend, const std::vector<size_t> &n_vars, const std::vector<FSlice> &inputs,
                                        const std::vector<FSliceMut> &arenas, FSliceMut scratch, const std::vector<B128> &batch_coeffs,
                                        const std::vector<B128> &sumcheck_challenges, const std::vector<B128> &gpa_challenges)
{
	size_t max_n = 0;
	for (size_t n : n_vars) max_n = std::max(max_n, n);
	if (n_vars.size() == inputs.size() && n_vars.size() == arenas.size() &&
	    (batch_coeffs.size() < max_n || gpa_challenges.size() < max_n || sumcheck_challenges.size() < max_n * (max_n ? max_n - 1 : 0) / 2))
		throw Error(Error::InputValidation, "too few transcript samples for the largest claim");
	ArrayTranscript tr({ArrayTranscript::stream(batch_coeffs), ArrayTranscript::stream(sumcheck_challenges), ArrayTranscript::stream(gpa_challenges)});
	return gkr_gpa_batch_prove(hal, backend, n_vars, inputs, arenas, scratch, tr);
}

} // namespace binius_amd
