// binius_amd/host/batch_prover.hpp -- C++ mirror of the reference's two batch sumcheck provers, over any prover with
// n_vars() / execute(batch_coeff) / fold(challenge) / finish():
//
//   FrontLoaded   crates/core/src/protocols/sumcheck/prove/front_loaded.rs:33-203 with the batch coefficients handed in
//                 (new_prebatched, :79-107): provers ascend by n_vars, all start in round 0, a prover finishes in the round that
//                 equals its n_vars (piop, evalcheck, zerocheck; gkr_gpa and flush as batches of one)
//   JoinBySize    crates/core/src/protocols/sumcheck/prove/batch_sumcheck.rs:102-199: provers descend by n_vars, a prover joins in
//                 the round where its n_vars equals the rounds left, all finish after the last round (gkr_exp)
//
// A round: execute every live prover, add its coefficients times its batch coefficient (RoundCoeffs, protocols/sumcheck/
// common.rs:108-150), drop the last coefficient (RoundCoeffs::truncate, common.rs:101-105) -- or, with `full_coeffs`, keep all of
// them padded to that many; then fold every live prover at the challenge.  The interface is stepwise (round_proof,
// receive_challenge, finish) for a caller that interleaves the rounds with something else; run() is the plain loop.  Coefficients
// and evaluations are returned; what is written to a transcript is the caller's.
#pragma once
#include <memory>

#include "sumcheck.hpp"
#include "transcript.hpp"

namespace binius_amd {

enum class BatchSchedule { FrontLoaded, JoinBySize };

struct BatchSumcheckOutput {
	std::vector<std::vector<B128>> round_proofs;      // per round
	std::vector<std::vector<B128>> multilinear_evals; // per prover, in finishing order
	std::vector<B128> challenges;                     // per round, as drawn (run over a TranscriptSource)
};

template <class Prover>
class SumcheckBatchProver {
public:
	SumcheckBatchProver(std::vector<std::unique_ptr<Prover>> provers, std::vector<B128> batch_coeffs, BatchSchedule schedule = BatchSchedule::FrontLoaded,
	                    size_t full_coeffs = 0)
	    : provers_(std::move(provers)), batch_coeffs_(std::move(batch_coeffs)), schedule_(schedule), full_coeffs_(full_coeffs)
	{
		const bool front = schedule_ == BatchSchedule::FrontLoaded;
		for (size_t i = 1; i < provers_.size(); i++)
			if (front ? provers_[i]->n_vars() < provers_[i - 1]->n_vars() : provers_[i]->n_vars() > provers_[i - 1]->n_vars()) throw SumcheckError("ClaimsOutOfOrder");
		if (batch_coeffs_.size() != provers_.size()) throw SumcheckError("IncorrectNumberOfBatchCoeffs");
		if (!provers_.empty()) total_rounds_ = front ? provers_.back()->n_vars() : provers_.front()->n_vars();
		if (front) live_end_ = provers_.size();
	}
	size_t total_rounds() const { return total_rounds_; }
	// the evaluations of the provers that have finished so far
	const std::vector<std::vector<B128>> &multilinear_evals() const { return multilinear_evals_; }

	std::vector<B128> round_proof()
	{
		update_live();
		std::vector<B128> round_coeffs;
		for (size_t i = live_begin_; i < live_end_; i++) {
			const std::vector<B128> prover_coeffs = provers_[i]->execute(batch_coeffs_[i]);
			if (round_coeffs.size() < prover_coeffs.size()) round_coeffs.resize(prover_coeffs.size(), B128::ZERO());
			for (size_t c = 0; c < prover_coeffs.size(); c++) round_coeffs[c] = round_coeffs[c] + prover_coeffs[c] * batch_coeffs_[i];
		}
		truncated_len_ = round_coeffs.empty() ? 0 : round_coeffs.size() - 1;
		if (full_coeffs_)
			round_coeffs.resize(full_coeffs_, B128::ZERO());
		else if (!round_coeffs.empty())
			round_coeffs.pop_back();
		return round_coeffs;
	}
	void receive_challenge(B128 challenge)
	{
		for (size_t i = live_begin_; i < live_end_; i++) provers_[i]->fold(challenge);
		round_++;
	}
	std::vector<std::vector<B128>> finish()
	{
		update_live();
		if (schedule_ == BatchSchedule::JoinBySize)
			for (; live_begin_ < provers_.size(); live_begin_++) multilinear_evals_.push_back(provers_[live_begin_]->finish());
		if (live_begin_ != provers_.size()) throw SumcheckError("ExpectedFold");
		return multilinear_evals_;
	}
	// every round with challenges[round], then finish
	BatchSumcheckOutput run(const B128 *challenges)
	{
		BatchSumcheckOutput out;
		for (size_t r = 0; r < total_rounds_; r++) {
			out.round_proofs.push_back(round_proof());
			receive_challenge(challenges[r]);
		}
		out.multilinear_evals = finish();
		return out;
	}

	// how many coefficients of the last round_proof() the transcript carries: all but the last of the batched polynomial
	// (RoundCoeffs::truncate) -- with `full_coeffs` fewer than were returned
	size_t truncated_len() const { return truncated_len_; }
	// BatchProver::run (front_loaded.rs:175-197; batch_sumcheck.rs:156-199) against a transcript: per round the evaluations of the
	// provers that finished (front_loaded.rs:109-120), the truncated round polynomial, then ONE sample (stream, first + round); after
	// the last round the evaluations of the provers that finish then.  Every output is what run(challenges) returns for the samples
	// drawn.  coeff_stream >= 0 (JoinBySize): the batch coefficients handed to the constructor are placeholders; prover i's is sampled
	// as (coeff_stream, coeff_first + i) in the round where it joins (batch_sumcheck.rs:143-151), those of the zero-variable provers
	// after the last round (:173-177).
	BatchSumcheckOutput run(TranscriptSource &tr, int stream, size_t first = 0, int coeff_stream = -1, size_t coeff_first = 0)
	{
		BatchSumcheckOutput out;
		size_t n_written = 0, n_coeffs = coeff_stream < 0 ? provers_.size() : 0;
		auto write_finished = [&] {
			for (; n_written < multilinear_evals_.size(); n_written++) tr.write_scalars(multilinear_evals_[n_written]);
		};
		auto sample_coeffs = [&](size_t end) {
			for (; n_coeffs < end; n_coeffs++) batch_coeffs_[n_coeffs] = tr.sample(coeff_stream, coeff_first + n_coeffs);
		};
		for (size_t r = 0; r < total_rounds_; r++) {
			update_live();
			sample_coeffs(live_end_);
			out.round_proofs.push_back(round_proof());
			write_finished();
			tr.write_scalars(out.round_proofs.back().data(), truncated_len_);
			out.challenges.push_back(tr.sample(stream, first + r));
			receive_challenge(out.challenges.back());
		}
		sample_coeffs(provers_.size());
		out.multilinear_evals = finish();
		write_finished();
		return out;
	}

private:
	// the provers [live_begin_, live_end_) take part in the round that begins
	void update_live()
	{
		if (schedule_ == BatchSchedule::FrontLoaded)
			for (; live_begin_ < provers_.size() && provers_[live_begin_]->n_vars() == round_; live_begin_++) {
				multilinear_evals_.push_back(provers_[live_begin_]->finish());
				provers_[live_begin_].reset(); // (front_loaded.rs:109-120 pops it: what it owns is released now, not after the last round)
			}
		else
			while (live_end_ < provers_.size() && provers_[live_end_]->n_vars() == total_rounds_ - round_) live_end_++;
	}
	std::vector<std::unique_ptr<Prover>> provers_;
	std::vector<B128> batch_coeffs_;
	BatchSchedule schedule_;
	size_t full_coeffs_;
	std::vector<std::vector<B128>> multilinear_evals_;
	size_t total_rounds_ = 0, round_ = 0, live_begin_ = 0, live_end_ = 0, truncated_len_ = 0;
};

// the front-loaded batch of ONE prover, every round: what a protocol step with a single sumcheck runs
template <class Prover>
inline BatchSumcheckOutput prove_batch_of_one(std::unique_ptr<Prover> prover, B128 batch_coeff, const B128 *challenges)
{
	std::vector<std::unique_ptr<Prover>> one;
	one.push_back(std::move(prover));
	return SumcheckBatchProver<Prover>(std::move(one), {batch_coeff}).run(challenges);
}
template <class Prover>
inline BatchSumcheckOutput prove_batch_of_one(std::unique_ptr<Prover> prover, B128 batch_coeff, TranscriptSource &tr, int stream, size_t first)
{
	std::vector<std::unique_ptr<Prover>> one;
	one.push_back(std::move(prover));
	return SumcheckBatchProver<Prover>(std::move(one), {batch_coeff}).run(tr, stream, first);
}

} // namespace binius_amd
