// binius_amd/host/ring_switch.hpp -- C++ mirror of the ring-switching reduction, ring_switch::prove (core/src/ring_switch/prove.rs:42-144):
//
//   mixing_coeffs                        prove.rs:79        the tensor expansion of the mixing challenges, on the host
//   compute_partial_evals                prove.rs:147-208   evaluate_partial_high of every committed column at its claim's suffix ("MLE Fold High"):
//                                                           one ops::eq_ind_partial_eval per distinct suffix, ONE bn_partial_eval_high_batch per distinct
//                                                           suffix over the distinct (column, suffix) pairs, one copy to the host per call
//   scale_tensor_elems                   prove.rs:210-225   TowerTensorAlgebra::scale_vertical, host
//   mix_tensor_elems_for_prefixes        prove.rs:227-250   host; a kappa mismatch inside a prefix is the reference's TowerLevelMismatch
//   compute_row_batched_sumcheck_evals   prove.rs:253-264   TensorAlgebra::fold_vertical (core/src/tensor_algebra.rs:139-152), host
//   make_ring_switch_eq_inds             prove.rs:116-124   ONE bn_ring_switch_eq_ind_batch for the transparents of ALL claims; its queries are the
//                                                           suffix tables the partial evaluations used
//
// The caller has done the oracle-set bookkeeping of EvalClaimSystem::new (ring_switch/common.rs:72-205) and hands in the committed
// columns, the suffix and prefix descriptors and the claims in the order the reference sorts them; the two sample_vec calls
// (prove.rs:68-69, 97) arrive as host arrays, like the challenges of the other provers.  memoized_data is not mirrored.
//
// What comes out, in transcript order: each prefix's mixed tensor element as 2^kappa scalars (prove.rs:90-94), row_batched_evals
// (prove.rs:104); then the transparents in claim order.  The PIOP sumcheck claim of claim i is (n_vars = its suffix's length, committed =
// its column, transparent = i, sum = row_batched_evals[i]) (prove.rs:127-138).
//
// Protocol bookkeeping only: every hypercube-sized operation is a call of the backend.
#pragma once
#include <algorithm>
#include <map>

#include "sumcheck.hpp"
#include "transcript.hpp"

namespace binius_amd {

struct RingSwitchSuffix { // EvalClaimSuffixDesc: the suffix pool[off .. off + len) and kappa
	uint32_t off = 0, len = 0, kappa = 0;
};
struct RingSwitchClaim { // PIOPSumcheckClaimDesc + eval_claim_to_prefix_desc_index
	uint32_t committed_idx = 0, suffix_desc_idx = 0, prefix_desc_idx = 0;
};
struct RingSwitchOutput {
	enum { PartialEvals = 0, TensorAlgebra = 1, EqInds = 2, NPhases = 3 };
	std::vector<B128> mixed_tensor_elems; // per prefix 2^kappa vertical elements, concatenated
	std::vector<B128> row_batched_evals;  // per claim
	std::vector<FSlice> transparents;     // per claim, 2^|suffix| elements
	double phase_ms[NPhases] = {};
};

// the identity of a suffix table: its slice of the pool
using RingSwitchSuffixKey = std::pair<uint32_t, uint32_t>;

// Exact: the tensor expansion of every distinct suffix, 2^kappa partial evaluations per distinct (column, suffix), one transparent per claim.
inline size_t ring_switch_scratch_elems(const std::vector<RingSwitchSuffix> &suffixes, const std::vector<RingSwitchClaim> &claims)
{
	std::map<RingSwitchSuffixKey, bool> tables;
	std::map<std::pair<uint32_t, RingSwitchSuffixKey>, bool> pairs;
	size_t total = 0;
	for (const RingSwitchClaim &c : claims) {
		if (c.suffix_desc_idx >= suffixes.size()) throw Error(Error::InputValidation, "a claim's suffix descriptor index is out of range");
		const RingSwitchSuffix &s = suffixes[c.suffix_desc_idx];
		if (s.len > BN_PE_MAX_VARS || s.kappa > 7) throw Error(Error::InputValidation, "a suffix descriptor is out of range");
		const RingSwitchSuffixKey key{s.off, s.len};
		if (tables.emplace(key, true).second) total += (size_t)1 << s.len;
		if (pairs.emplace(std::make_pair(c.committed_idx, key), true).second) total += (size_t)1 << s.kappa;
		total += (size_t)1 << s.len;
	}
	return total;
}

// limb i (2^(7 - kappa) bits, at most 64) of a field element
inline uint64_t tower_limb(B128 e, size_t i, size_t kappa)
{
	const size_t w = (size_t)1 << (7 - kappa), bit = i * w;
	const uint64_t word = bit < 64 ? e.lo : e.hi;
	return w == 64 ? word : (word >> (bit & 63)) & (((uint64_t)1 << w) - 1);
}

// TensorAlgebra::fold_vertical (tensor_algebra.rs:139-152): the square transpose of the 2^kappa x 2^kappa limb matrix, then the inner
// product with the first 2^kappa coefficients
inline B128 tower_fold_vertical(const std::vector<B128> &elems, size_t kappa, const std::vector<B128> &coeffs)
{
	const size_t n = (size_t)1 << kappa;
	if (kappa == 0) return elems[0] * coeffs[0];
	const size_t w = (size_t)1 << (7 - kappa);
	B128 acc = B128::ZERO();
	for (size_t r = 0; r < n; r++) {
		B128 row = B128::ZERO(); // limb c of the transposed row r = limb r of element c
		for (size_t c = 0; c < n; c++) {
			const uint64_t v = tower_limb(elems[c], r, kappa);
			const size_t bit = c * w;
			if (bit < 64)
				row.lo |= v << bit;
			else
				row.hi |= v << (bit - 64);
		}
		acc += row * coeffs[r];
	}
	return acc;
}

// Schedule (ring_switch/prove.rs:68-104): sample the ceil(log2 n_claims) mixing challenges (stream RingSwitchMixing); write per prefix its
// 2^kappa mixed vertical elements; sample the max-kappa row-batch challenges (stream RingSwitchRowBatch); write the n_claims row-batched
// evaluations.  n_mixing / n_row_batch: what the caller of the array form handed in (checked against the claims), or -1.
enum { RingSwitchMixing = 0, RingSwitchRowBatch = 1 };
inline RingSwitchOutput ring_switch_prove(ComputeLayer &hal, const std::vector<bn_pe_column> &columns, const std::vector<B128> &pool,
                                          const std::vector<RingSwitchSuffix> &suffixes, const std::vector<uint32_t> &prefix_kappas,
                                          const std::vector<RingSwitchClaim> &claims, TranscriptSource &tr, FSliceMut scratch, long n_mixing = -1, long n_row_batch = -1)
{
	// ---- everything is checked before the first device call
	size_t log_claims = 0, max_kappa = 0;
	while (((size_t)1 << log_claims) < claims.size()) log_claims++;
	if (n_mixing >= 0 && (size_t)n_mixing != log_claims) throw Error(Error::InputValidation, "ring switch: ceil(log2 n_claims) mixing challenges");
	for (const RingSwitchSuffix &s : suffixes) {
		if (s.kappa > 7 || s.len > BN_PE_MAX_VARS) throw Error(Error::InputValidation, "a suffix descriptor is out of range");
		if ((size_t)s.off + s.len > pool.size()) throw Error(Error::InputValidation, "a suffix leaves the point pool");
	}
	for (const uint32_t k : prefix_kappas)
		if (k > 7) throw Error(Error::InputValidation, "a prefix descriptor's kappa is out of range");
	for (const RingSwitchClaim &c : claims) {
		if (c.committed_idx >= columns.size() || c.suffix_desc_idx >= suffixes.size() || c.prefix_desc_idx >= prefix_kappas.size())
			throw Error(Error::InputValidation, "a claim's index is out of range");
		const bn_pe_column &col = columns[c.committed_idx];
		const RingSwitchSuffix &s = suffixes[c.suffix_desc_idx];
		if (!col.d_evals) throw Error(Error::InputValidation, "null committed column");
		if (col.tower_level > 7 || col.n_vars + col.tower_level < 7) throw Error(Error::InputValidation, "a committed column is at least one 128-bit element: n_vars + tower_level >= 7");
		if (s.kappa != 7 - col.tower_level) throw Error(Error::InputValidation, "a claim's kappa is 7 - the tower level of its column");
		if (col.n_vars != s.kappa + s.len) throw Error(Error::InputValidation, "a claim's suffix has n_vars - kappa coordinates");
		if (prefix_kappas[c.prefix_desc_idx] != s.kappa) throw Error(Error::InputValidation, "TowerLevelMismatch: the claims of a prefix share its kappa");
		max_kappa = std::max<size_t>(max_kappa, s.kappa);
	}
	if (n_row_batch >= 0 && (size_t)n_row_batch != max_kappa) throw Error(Error::InputValidation, "ring switch: max kappa row-batch challenges");
	if (scratch.len_ < ring_switch_scratch_elems(suffixes, claims)) throw Error(Error::InputValidation, "scratch holds fewer than ring_switch_scratch_elems elements");
	RingSwitchOutput out;
	if (claims.empty()) {
		for (const uint32_t k : prefix_kappas) out.mixed_tensor_elems.resize(out.mixed_tensor_elems.size() + ((size_t)1 << k), B128::ZERO());
		tr.write_scalars(out.mixed_tensor_elems);
		return out;
	}
	DeviceBumpAllocator alloc(scratch);
	const std::vector<B128> mixing_challenges = tr.sample_vec(RingSwitchMixing, 0, log_claims); // (:68-69)
	const std::vector<B128> mixing_coeffs = eq_expand(mixing_challenges.data(), mixing_challenges.size()); // (:79)

	// ---- compute_partial_evals: distinct suffixes expanded once, the distinct columns of a suffix in one call
	const auto t_begin = std::chrono::steady_clock::now();
	struct SuffixJob {
		FSlice query;
		uint32_t len = 0;
		std::vector<bn_pe_column> cols;
		std::vector<uint32_t> col_idx;
		std::vector<size_t> at; // where the column's 2^kappa elements begin in the job's block
		size_t elems = 0;
		std::vector<B128> host;
	};
	std::map<RingSwitchSuffixKey, SuffixJob> jobs;
	for (const RingSwitchClaim &c : claims) {
		const RingSwitchSuffix &s = suffixes[c.suffix_desc_idx];
		const RingSwitchSuffixKey key{s.off, s.len};
		auto job = jobs.find(key);
		if (job == jobs.end()) {
			const FSliceMut q = ops::eq_ind_partial_eval(hal, alloc, std::vector<B128>(pool.begin() + s.off, pool.begin() + s.off + s.len));
			job = jobs.emplace(key, SuffixJob{}).first;
			job->second.query = ComputeMemory::as_const(q);
			job->second.len = s.len;
		}
		SuffixJob &j = job->second;
		if (std::find(j.col_idx.begin(), j.col_idx.end(), c.committed_idx) != j.col_idx.end()) continue;
		j.col_idx.push_back(c.committed_idx);
		j.cols.push_back(columns[c.committed_idx]);
		j.at.push_back(j.elems);
		j.elems += (size_t)1 << s.kappa;
	}
	for (auto &kv : jobs) {
		SuffixJob &j = kv.second;
		FSliceMut block = alloc.alloc(j.elems);
		std::vector<void *> outs;
		for (const size_t at : j.at) outs.push_back(static_cast<char *>(block.ptr) + 16 * at);
		check(bn_partial_eval_high_batch(hal.raw_ctx(), j.cols.data(), (uint32_t)j.cols.size(), j.query.ptr, j.len, outs.data()));
		j.host.resize(j.elems);
		hal.copy_d2h(ComputeMemory::as_const(block), j.host);
	}
	const auto t_pe = std::chrono::steady_clock::now();
	out.phase_ms[RingSwitchOutput::PartialEvals] = elapsed_ms(t_begin, t_pe);

	// ---- scale and mix per prefix; the mixed elements are written before the row-batch challenges are drawn (:90-97)
	std::vector<std::vector<B128>> mixed, scaled(claims.size());
	for (const uint32_t k : prefix_kappas) mixed.emplace_back((size_t)1 << k, B128::ZERO());
	out.row_batched_evals.resize(claims.size());
	for (size_t i = 0; i < claims.size(); i++) {
		const RingSwitchClaim &c = claims[i];
		const RingSwitchSuffix &s = suffixes[c.suffix_desc_idx];
		const SuffixJob &j = jobs.at(RingSwitchSuffixKey{s.off, s.len});
		const size_t at = j.at[std::find(j.col_idx.begin(), j.col_idx.end(), c.committed_idx) - j.col_idx.begin()];
		std::vector<B128> elems(j.host.begin() + at, j.host.begin() + at + ((size_t)1 << s.kappa));
		for (B128 &e : elems) e = e * mixing_coeffs[i]; // scale_vertical
		std::vector<B128> &m = mixed[c.prefix_desc_idx];
		for (size_t v = 0; v < elems.size(); v++) m[v] += elems[v];
		scaled[i] = std::move(elems);
	}
	for (const std::vector<B128> &m : mixed) out.mixed_tensor_elems.insert(out.mixed_tensor_elems.end(), m.begin(), m.end());
	tr.write_scalars(out.mixed_tensor_elems);
	// ---- fold with the row-batch coefficients
	const std::vector<B128> row_batch_challenges = tr.sample_vec(RingSwitchRowBatch, 0, max_kappa);                   // (:97)
	const std::vector<B128> row_batch_coeffs = eq_expand(row_batch_challenges.data(), row_batch_challenges.size()); // (:98-100)
	for (size_t i = 0; i < claims.size(); i++) out.row_batched_evals[i] = tower_fold_vertical(scaled[i], suffixes[claims[i].suffix_desc_idx].kappa, row_batch_coeffs);
	tr.write_scalars(out.row_batched_evals); // (:104)
	const auto t_ta = std::chrono::steady_clock::now();
	out.phase_ms[RingSwitchOutput::TensorAlgebra] = elapsed_ms(t_pe, t_ta);

	// ---- make_ring_switch_eq_inds: every claim's transparent in one launch
	std::vector<bn_rs_job> rs(claims.size());
	std::vector<void *> rs_outs(claims.size());
	for (size_t i = 0; i < claims.size(); i++) {
		const RingSwitchSuffix &s = suffixes[claims[i].suffix_desc_idx];
		FSliceMut t = alloc.alloc((size_t)1 << s.len);
		rs[i] = bn_rs_job{jobs.at(RingSwitchSuffixKey{s.off, s.len}).query.ptr, s.len, s.kappa, mixing_coeffs[i].raw()};
		rs_outs[i] = t.ptr;
		out.transparents.push_back(ComputeMemory::as_const(t));
	}
	std::vector<bn_f128> raw_coeffs(row_batch_coeffs.size());
	to_raw(row_batch_coeffs, raw_coeffs.data());
	check(bn_ring_switch_eq_ind_batch(hal.raw_ctx(), rs.data(), (uint32_t)rs.size(), raw_coeffs.data(), (uint32_t)raw_coeffs.size(), rs_outs.data()));
	out.phase_ms[RingSwitchOutput::EqInds] = elapsed_ms(t_ta);
	return out;
}
inline RingSwitchOutput ring_switch_prove(ComputeLayer &hal, const std::vector<bn_pe_column> &columns, const std::vector<B128> &pool,
                                          const std::vector<RingSwitchSuffix> &suffixes, const std::vector<uint32_t> &prefix_kappas,
                                          const std::vector<RingSwitchClaim> &claims, const std::vector<B128> &mixing_challenges,
                                          const std::vector<B128> &row_batch_challenges, FSliceMut scratch)
{
	ArrayTranscript tr({ArrayTranscript::stream(mixing_challenges), ArrayTranscript::stream(row_batch_challenges)});
	return ring_switch_prove(hal, columns, pool, suffixes, prefix_kappas, claims, tr, scratch, (long)mixing_challenges.size(), (long)row_batch_challenges.size());
}

} // namespace binius_amd
