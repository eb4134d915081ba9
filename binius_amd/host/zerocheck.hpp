// binius_amd/host/zerocheck.hpp -- C++ mirror of the batched univariate-skip zerocheck prover, sumcheck::prove::batch_zerocheck::
// batch_prove (crates/core/src/protocols/sumcheck/prove/batch_zerocheck.rs:166-293) over ZerocheckProverImpl (prove/zerocheck.rs:
// 121-516), as constraint_system::prove calls it (core/src/constraint_system/prove.rs:446-501) for the domain field B8 (the 0..=3 arm
// of :484).  The transcript's samples are handed in.
//
//   execute_univariate_round   prove/zerocheck.rs:316-381    bn_zerocheck_univariate_evals per table (per composition), batched on the
//                                                             host with the powers of the table's coefficient, times the coefficient
//                                                             again (batch_zerocheck.rs:198-206)
//   ZerocheckUnivariateEvalsOutput::fold   univariate.rs:139-193   host: the Lagrange coefficients of the subcube and of the whole
//                                                             domain at the univariate challenge, the claimed sums
//   fold_univariate_round      prove/zerocheck.rs:384-470    ONE bn_univariate_fold_batch over the columns of ALL tables, then one
//                                                             EqIndPointProver (eq_ind.hpp) per table over max(n, k) - k variables;
//                                                             its indicator table is the expansion of all its challenges but the
//                                                             last (fold_partial_eq_ind, High-to-Low, of the univariate round's table)
//   front_loaded::BatchProver::new_prebatched   prove/front_loaded.rs:78-198   SumcheckBatchProver (batch_prover.hpp): every prover starts in round 0, its round polynomial
//                                                             times its PRE-sampled coefficient; a prover finishes in the round that
//                                                             equals its number of variables (with none: at once)
//   project_to_skipped_variables   prove/zerocheck.rs:472-516   ONE bn_partial_eval_high_batch per table: the original columns at the
//                                                             last n - k unskipped challenges, 2^k values each
//   univariatizing_reduction_prover   batch_zerocheck.rs:115-154, zerocheck.rs:199-227   RegularSumcheckProver over k variables, High-to-
//                                                             Low, one bivariate product claim per column against the Lagrange-
//                                                             coefficient multilinear: at most a few hundred multilinears of at most
//                                                             256 elements -- host arithmetic (the reference takes its portable
//                                                             backend here too)
//
// A table of n < k variables is padded high by repetition to k variables on the host (high_pad_small_multilinear, prove/zerocheck.rs:
// 79-119); its projection is the padded column itself.  Columns of less than one 16-byte element are projected on the host as well.
// Round polynomials are returned with ALL their coefficients (the transcript carries the truncated form), the multilinear rounds'
// padded to Dmax + 2, Dmax = max(2, largest degree of the batch), as bnh_eqind_sumcheck_prove pads.
//
// tower = true (bnh_zerocheck_batch_prove_tower) takes every arm of :483-490: columns at level 0 or 3 .. 7, constants anywhere in
// B128.  A table's arm is the largest of its column levels and of the levels of its compositions' constants, at least 3 (:458-467):
// its univariate round is bn_zerocheck_univariate_evals at base 3 and bn_zerocheck_univariate_evals_base above.  The columns of level
// 0 / 3 of ALL tables stay in the ONE bn_univariate_fold_batch; a wider column takes bn_fold_right with the Lagrange coefficients,
// which the header defines the fold's result as -- the coefficients are uploaded once per proof (a batched wide fold: DESIGN.md 7).
// The projection's bn_partial_eval_high_batch takes every level.  Padding and the columns of less than one element are done on the
// host for every level.
#pragma once
#include <chrono>
#include <cstring>

#include "batch_prover.hpp"
#include "eq_ind.hpp"

namespace binius_amd {

struct ZerocheckColumn {
	const void *d_evals = nullptr; // TRANSPARENT, packed as bn_hal_multilinear says
	uint32_t tower_level = 0;      // 0 (B1) or 3 (B8); with tower = true: 0 or 3 .. 7
};

struct ZerocheckTable {
	size_t n_vars = 0;
	std::vector<ZerocheckColumn> columns;
	std::vector<std::vector<bn_step>> base_compositions; // over the table's base field (B8 without tower): the univariate round
	std::vector<EqIndComposition> compositions;          // the same circuits over B128, their leading forms and degrees: the multilinear rounds
};

struct ZerocheckBatchOutput {
	std::vector<B128> message;                           // D - 2^k values, D = (largest degree) 2^k
	std::vector<std::vector<B128>> round_coeffs;         // max_n - k rounds of Dmax + 2 coefficients
	std::vector<std::vector<B128>> final_evals;          // per table, finishing (= input) order: the columns', then the indicator's
	std::vector<std::vector<B128>> reduction_round_coeffs; // k rounds of 3 coefficients
	std::vector<B128> reduction_final_evals;             // every column's, then the Lagrange-coefficient multilinear's
	std::vector<B128> skipped_challenges, unskipped_challenges, concat_multilinear_evals; // BatchZerocheckOutput (zerocheck.rs:140-150)
	enum Phase { Univariate = 0, Fold = 1, Multilinear = 2, Projection = 3, Reduction = 4, NPhases = 5 };
	double phase_ms[NPhases] = {};      // wall time
	uint64_t phase_calls[NPhases] = {}; // device-op calls of the C ABI the phase made itself (copies and the provers' backend calls not counted)
};

// Device scratch of zerocheck_batch_prove, in elements: per table the padded columns (n < k), the univariate round's indicator table,
// the folded columns, the eq-ind prover's indicator table, the projection's query and its outputs.
inline size_t zerocheck_batch_scratch_elems(const std::vector<size_t> &n_vars, const std::vector<size_t> &n_cols, size_t k)
{
	size_t total = 0;
	for (size_t p = 0; p < n_vars.size(); p++) {
		const size_t n_eff = n_vars[p] > k ? n_vars[p] : k, nr = n_eff - k;
		if (n_vars[p] < k) total += n_cols[p] * 16;
		total += ((size_t)1 << nr) + (n_cols[p] << nr) + (nr ? (size_t)1 << (nr - 1) : 0);
		if (n_vars[p] >= k) total += ((size_t)1 << nr) + (n_cols[p] << k);
	}
	return total;
}

namespace zerocheck_detail {
inline size_t column_elems(size_t n_vars, uint32_t level);
}

// The same for zerocheck_batch_prove with tower = true, which depends on the levels: a padded column takes the elements its level
// needs (a level-7 column at k = 7: 128), and a batch with a column above level 3 holds the 2^k Lagrange coefficients of the wide folds.
inline size_t zerocheck_batch_scratch_elems_tower(const std::vector<size_t> &n_vars, const std::vector<std::vector<uint32_t>> &levels, size_t k)
{
	size_t total = 0;
	bool wide = false;
	for (size_t p = 0; p < n_vars.size(); p++) {
		const size_t n_eff = n_vars[p] > k ? n_vars[p] : k, nr = n_eff - k, n_cols = levels[p].size();
		for (uint32_t level : levels[p]) {
			wide = wide || level > 3;
			if (n_vars[p] < k) total += zerocheck_detail::column_elems(k, level);
		}
		total += ((size_t)1 << nr) + (n_cols << nr) + (nr ? (size_t)1 << (nr - 1) : 0);
		if (n_vars[p] >= k) total += ((size_t)1 << nr) + (n_cols << k);
	}
	return total + (wide ? (size_t)1 << k : 0);
}

namespace zerocheck_detail {

// B8 in the tower basis: products and inverses as tables, built once from the scalar field (a B8 element embeds as itself)
struct B8Tables {
	uint8_t mul[256][256];
	uint8_t inv[256];
	B8Tables()
	{
		for (unsigned a = 0; a < 256; a++)
			for (unsigned b = a; b < 256; b++) mul[a][b] = mul[b][a] = (uint8_t)(B128(a) * B128(b)).lo;
		inv[0] = 0;
		for (unsigned a = 1; a < 256; a++)
			for (unsigned b = 1; b < 256; b++)
				if (mul[a][b] == 1) inv[a] = (uint8_t)b;
	}
	static const B8Tables &get()
	{
		static const B8Tables t;
		return t;
	}
};

// EvaluationDomain::lagrange_evals over omega_0 .. omega_{n-1}, omega_j = the B8 element whose tower bits are j, at z in B128:
// L_j(z) = prod_{q != j} (z - omega_q) / (omega_j - omega_q).  The numerators from prefix and suffix products, the denominators in B8.
inline std::vector<B128> lagrange_evals(size_t n, B128 z)
{
	const B8Tables &t = B8Tables::get();
	std::vector<B128> prefix(n + 1, B128::ONE()), out(n);
	for (size_t q = 0; q < n; q++) prefix[q + 1] = prefix[q] * (z + B128(q));
	B128 suffix = B128::ONE();
	for (size_t j = n; j-- > 0;) {
		uint8_t den = 1;
		for (size_t q = 0; q < n; q++)
			if (q != j) den = t.mul[den][j ^ q];
		out[j] = prefix[j] * suffix * B128(t.inv[den]);
		suffix = suffix * (z + B128(j));
	}
	return out;
}

// value i of a packed column of at most 2^11 bits held on the host
inline uint8_t packed_value(const std::vector<B128> &col, uint32_t level, size_t i)
{
	const uint8_t *raw = reinterpret_cast<const uint8_t *>(col.data());
	return level == 0 ? (raw[i >> 3] >> (i & 7)) & 1 : raw[i];
}

inline size_t column_elems(size_t n_vars, uint32_t level) { return n_vars + level <= 7 ? 1 : (size_t)1 << (n_vars + level - 7); }

// value i of a packed column of any level held on the host, as a field element (a subfield element embeds as itself)
inline B128 packed_element(const std::vector<B128> &col, uint32_t level, size_t i)
{
	if (level <= 3) return B128(packed_value(col, level, i));
	uint64_t w[2] = {0, 0};
	std::memcpy(w, reinterpret_cast<const uint8_t *>(col.data()) + (i << (level - 3)), (size_t)1 << (level - 3));
	return B128(w[0], w[1]);
}

// binary_tower_level() of a constant: the smallest level whose field holds it
inline uint32_t const_level(const bn_f128 &c)
{
	if (c.hi) return 7;
	uint32_t level = 0;
	while (level < 6 && (c.lo >> (1u << level))) level++;
	return level;
}

// the arm of a table (core/src/constraint_system/prove.rs:458-467): the largest column level and composition level, 0 .. 3 => 3
inline uint32_t table_base(const ZerocheckTable &t)
{
	uint32_t base = 3;
	for (const ZerocheckColumn &c : t.columns) base = c.tower_level > base ? c.tower_level : base;
	for (const auto &steps : t.base_compositions)
		for (const bn_step &st : steps)
			if (st.kind == BN_STEP_CONST) base = const_level(st.cst) > base ? const_level(st.cst) : base;
	return base;
}

} // namespace zerocheck_detail

// The transcript's streams, as the array form names them.
// Schedule (constraint_system/prove.rs:470; batch_zerocheck.rs:193-272): sample the max_n - k zerocheck challenges; sample the n_tables
// batch coefficients; write the univariate round's message (D - 2^k scalars); sample the univariate challenge; the max_n - k multilinear
// rounds as a front-loaded batch (per round the evaluations of the tables that finished, the truncated round polynomial, ONE sample;
// then the last tables' evaluations); sample the reduction's batch coefficient; k rounds of write 2 coefficients / sample 1; write the
// reduction's evaluations (every column's, then the Lagrange multilinear's).
enum { ZerocheckChallenges = 0, ZerocheckBatchCoeffs = 1, ZerocheckUnivariateChallenge = 2, ZerocheckSumcheckChallenges = 3, ZerocheckReductionBatchCoeff = 4,
       ZerocheckReductionChallenges = 5 };
inline ZerocheckBatchOutput zerocheck_batch_prove(ComputeLayer &hal, const std::vector<ZerocheckTable> &tables, size_t skip_rounds, TranscriptSource &tr, FSliceMut scratch,
                                                  bool tower = false)
{
	using namespace zerocheck_detail;
	using Out = ZerocheckBatchOutput;
	const size_t k = skip_rounds, K = (size_t)1 << k;
	// ---- validation, up front
	if (tables.empty()) throw Error(Error::InputValidation, "zerocheck: no table");
	if (k < 1 || k > 8) throw Error(Error::InputValidation, "zerocheck: skip_rounds out of range (1 .. 8)");
	size_t d_top = 0;
	std::vector<size_t> nv, nc;
	std::vector<std::vector<uint32_t>> col_levels;
	bool any_wide = false;
	for (size_t p = 0; p < tables.size(); p++) {
		const ZerocheckTable &t = tables[p];
		if (p && t.n_vars < tables[p - 1].n_vars) throw Error(Error::InputValidation, "ClaimsOutOfOrder: tables ascend by number of variables");
		if (t.n_vars > BN_PE_MAX_VARS) throw Error(Error::InputValidation, "zerocheck: n_vars out of range");
		if (t.base_compositions.size() != t.compositions.size()) throw Error(Error::InputValidation, "zerocheck: one B8 composition per composition");
		for (const ZerocheckColumn &c : t.columns) {
			if (!c.d_evals) throw Error(Error::InputValidation, "zerocheck: null column");
			if (!tower && c.tower_level != 0 && c.tower_level != 3) throw Error(Error::InputValidation, "zerocheck: tower level must be 0 or 3");
			if (tower && c.tower_level != 0 && (c.tower_level < 3 || c.tower_level > 7)) throw Error(Error::InputValidation, "zerocheck: tower level must be 0 or 3 .. 7");
			any_wide = any_wide || c.tower_level > 3;
		}
		col_levels.emplace_back();
		for (const ZerocheckColumn &c : t.columns) col_levels.back().push_back(c.tower_level);
		for (const EqIndComposition &c : t.compositions) {
			if (c.degree < 1 || (c.degree << k) > 256) throw Error(Error::InputValidation, "zerocheck: a composition's degree d needs 1 <= d and d 2^k <= 256");
			d_top = c.degree > d_top ? c.degree : d_top;
		}
		nv.push_back(t.n_vars);
		nc.push_back(t.columns.size());
	}
	const size_t max_n = tables.back().n_vars;
	if (k > max_n) throw Error(Error::InputValidation, "IncorrectSkippedRoundsCount: skip_rounds exceeds the largest n_vars");
	const size_t rounds = max_n - k, D = d_top << k, d_max = d_top > 2 ? d_top : 2;
	if (!tower && scratch.len_ < zerocheck_batch_scratch_elems(nv, nc, k)) throw Error(Error::InputValidation, "scratch holds fewer than zerocheck_batch_scratch_elems elements");
	if (tower && scratch.len_ < zerocheck_batch_scratch_elems_tower(nv, col_levels, k))
		throw Error(Error::InputValidation, "scratch holds fewer than zerocheck_batch_scratch_elems_tower elements");

	Out out;
	Mi355xBackend backend(hal);
	DeviceBumpAllocator alloc(scratch);
	const std::vector<B128> zerocheck_challenges = tr.sample_vec(ZerocheckChallenges, 0, rounds);
	const std::vector<B128> batch_coeffs = tr.sample_vec(ZerocheckBatchCoeffs, 0, tables.size());
	struct Prover {
		size_t n_eff = 0, nr = 0;
		std::vector<const void *> cols;                // the columns the univariate round and the fold read (padded copies for n < k)
		std::vector<std::vector<B128>> host_cols;      // n < k: the padded columns, packed
		std::vector<B128> challenges;                  // the suffix of the zerocheck challenges (constraint_system/prove.rs:470)
		std::vector<std::vector<B128>> round_evals;    // per composition, D - 2^k values
		std::vector<FSlice> folded;
	};
	std::vector<Prover> ps(tables.size());

	// ---- the univariate round
	auto t0 = std::chrono::steady_clock::now();
	out.message.assign(D - K, B128::ZERO());
	for (size_t p = 0; p < tables.size(); p++) {
		const ZerocheckTable &t = tables[p];
		Prover &pr = ps[p];
		pr.n_eff = t.n_vars > k ? t.n_vars : k;
		pr.nr = pr.n_eff - k;
		pr.challenges.assign(zerocheck_challenges.begin() + (rounds - pr.nr), zerocheck_challenges.end());
		for (const ZerocheckColumn &c : t.columns) {
			if (t.n_vars >= k) {
				pr.cols.push_back(c.d_evals);
				continue;
			}
			// high_pad_small_multilinear: 2^(k - n) copies of the 2^n values
			std::vector<B128> small(column_elems(t.n_vars, c.tower_level)), padded(column_elems(k, c.tower_level));
			hal.copy_d2h(FSlice{c.d_evals, small.size()}, small);
			uint8_t *raw = reinterpret_cast<uint8_t *>(padded.data());
			for (size_t i = 0; i < K; i++) {
				const size_t src = i & (((size_t)1 << t.n_vars) - 1);
				if (c.tower_level == 0)
					raw[i >> 3] |= (uint8_t)(packed_value(small, 0, src) << (i & 7));
				else // (values of 2^(level - 3) bytes)
					std::memcpy(raw + (i << (c.tower_level - 3)), reinterpret_cast<const uint8_t *>(small.data()) + (src << (c.tower_level - 3)), (size_t)1 << (c.tower_level - 3));
			}
			FSliceMut d = alloc.alloc(padded.size());
			hal.copy_h2d(padded, d);
			pr.cols.push_back(d.ptr);
			pr.host_cols.push_back(std::move(padded));
		}
		const FSliceMut eq = ops::eq_ind_partial_eval(hal, alloc, pr.challenges, false);
		std::vector<bn_hal_multilinear> mls;
		for (size_t c = 0; c < t.columns.size(); c++) {
			bn_hal_multilinear m{};
			m.kind = BN_HAL_ML_TRANSPARENT;
			m.tower_level = t.columns[c].tower_level;
			m.d_evals = pr.cols[c];
			m.len = column_elems(pr.n_eff, t.columns[c].tower_level);
			m.n_vars_ml = (uint32_t)pr.n_eff;
			mls.push_back(m);
		}
		std::vector<bn_step> steps;
		std::vector<uint32_t> offsets{0}, degrees;
		for (size_t c = 0; c < t.compositions.size(); c++) {
			steps.insert(steps.end(), t.base_compositions[c].begin(), t.base_compositions[c].end());
			offsets.push_back((uint32_t)steps.size());
			degrees.push_back((uint32_t)t.compositions[c].degree);
		}
		std::vector<B128> per(t.compositions.size() * (D - K) + 1);
		if (!t.compositions.empty()) {
			const uint32_t base = tower ? table_base(t) : 3;
			if (base == 3)
				check(bn_zerocheck_univariate_evals(hal.raw_ctx(), (uint32_t)pr.n_eff, (uint32_t)k, mls.data(), (uint32_t)mls.size(), steps.data(), offsets.data(), degrees.data(),
				                                    (uint32_t)t.compositions.size(), eq.ptr, eq.len_, (uint32_t)D, nullptr, reinterpret_cast<bn_f128 *>(per.data())));
			else
				check(bn_zerocheck_univariate_evals_base(hal.raw_ctx(), base, (uint32_t)pr.n_eff, (uint32_t)k, mls.data(), (uint32_t)mls.size(), steps.data(), offsets.data(),
				                                         degrees.data(), (uint32_t)t.compositions.size(), eq.ptr, eq.len_, (uint32_t)D, nullptr,
				                                         reinterpret_cast<bn_f128 *>(per.data())));
			out.phase_calls[Out::Univariate] += 2 + (pr.nr ? 1 : 0);
		}
		// the powers of the coefficient (prove/zerocheck.rs:354-370), times the coefficient (batch_zerocheck.rs:198-206)
		B128 scale = batch_coeffs[p];
		for (size_t c = 0; c < t.compositions.size(); c++) {
			pr.round_evals.emplace_back(per.begin() + c * (D - K), per.begin() + (c + 1) * (D - K));
			for (size_t j = 0; j < D - K; j++) out.message[j] += scale * pr.round_evals[c][j];
			scale = scale * batch_coeffs[p];
		}
	}
	out.phase_ms[Out::Univariate] = elapsed_ms(t0);
	tr.write_scalars(out.message); // (batch_zerocheck.rs:209-210)
	const B128 univariate_challenge = tr.sample(ZerocheckUnivariateChallenge, 0);

	// ---- ZerocheckUnivariateEvalsOutput::fold and fold_univariate_round
	t0 = std::chrono::steady_clock::now();
	const std::vector<B128> l_sub = lagrange_evals(K, univariate_challenge), l_full = lagrange_evals(D, univariate_challenge);
	std::vector<bn_pe_column> fold_cols;
	std::vector<void *> fold_outs;
	FSliceMut d_l_sub{nullptr, 0}; // the coefficients of the wide folds, uploaded once per proof
	if (any_wide) {
		d_l_sub = alloc.alloc(K);
		hal.copy_h2d(l_sub, d_l_sub);
	}
	for (size_t p = 0; p < tables.size(); p++)
		for (size_t c = 0; c < tables[p].columns.size(); c++) {
			const uint32_t level = tables[p].columns[c].tower_level;
			const size_t n_out = (size_t)1 << ps[p].nr;
			FSliceMut o = alloc.alloc(n_out);
			ps[p].folded.push_back(ComputeMemory::as_const(o));
			if (level <= 3) {
				fold_cols.push_back(bn_pe_column{ps[p].cols[c], level, (uint32_t)ps[p].n_eff});
				fold_outs.push_back(o.ptr);
			} else if (ps[p].n_eff + level < 7) {
				// less than one 16-byte element (then n_eff = k and there is one output): on the host
				std::vector<B128> small(1), folded(n_out, B128::ZERO());
				hal.copy_d2h(FSlice{ps[p].cols[c], 1}, small);
				for (size_t i = 0; i < (n_out << k); i++) folded[i >> k] += l_sub[i & (K - 1)] * packed_element(small, level, i);
				hal.copy_h2d(folded, o);
			} else {
				check(bn_fold_right(hal.raw_ctx(), ps[p].cols[c], column_elems(ps[p].n_eff, level), level, d_l_sub.ptr, K, o.ptr, n_out));
				out.phase_calls[Out::Fold] += 1;
			}
		}
	if (!tower || !fold_cols.empty()) { // (a batch of wide columns only makes no call)
		check(bn_univariate_fold_batch(hal.raw_ctx(), fold_cols.data(), (uint32_t)fold_cols.size(), (uint32_t)k, reinterpret_cast<const bn_f128 *>(l_sub.data()), fold_outs.data()));
		out.phase_calls[Out::Fold] += fold_cols.empty() ? 0 : 1;
	}
	out.phase_ms[Out::Fold] = elapsed_ms(t0);

	// ---- the multilinear rounds: front-loaded, pre-batched
	t0 = std::chrono::steady_clock::now();
	std::vector<std::unique_ptr<EqIndPointProver>> provers;
	for (size_t p = 0; p < tables.size(); p++) {
		Prover &pr = ps[p];
		std::vector<B128> sums;
		for (const auto &evals : pr.round_evals) {
			B128 s = B128::ZERO();
			for (size_t j = 0; j < D - K; j++) s += evals[j] * l_full[K + j];
			sums.push_back(s);
		}
		// (no remaining round: the folded columns are single values, the indicator's evaluation is ONE)
		provers.push_back(std::make_unique<EqIndPointProver>(hal, backend, alloc, pr.nr, pr.folded, tables[p].compositions, std::move(sums), pr.challenges));
	}
	// all coefficients of a round polynomial, padded to Dmax + 2
	BatchSumcheckOutput res = SumcheckBatchProver<EqIndPointProver>(std::move(provers), batch_coeffs, BatchSchedule::FrontLoaded, d_max + 2).run(tr, ZerocheckSumcheckChallenges);
	out.round_coeffs = std::move(res.round_proofs);
	out.final_evals = std::move(res.multilinear_evals);
	out.phase_ms[Out::Multilinear] = elapsed_ms(t0);

	// ---- project_to_skipped_variables
	t0 = std::chrono::steady_clock::now();
	out.unskipped_challenges.assign(res.challenges.rbegin(), res.challenges.rend());
	std::vector<std::vector<B128>> projected; // every column of every table, 2^k values
	for (size_t p = 0; p < tables.size(); p++) {
		const ZerocheckTable &t = tables[p];
		const Prover &pr = ps[p];
		const size_t first = projected.size();
		projected.resize(first + t.columns.size(), std::vector<B128>(K));
		if (t.n_vars < k) {
			for (size_t c = 0; c < t.columns.size(); c++)
				for (size_t u = 0; u < K; u++) projected[first + c][u] = packed_element(pr.host_cols[c], t.columns[c].tower_level, u);
			continue;
		}
		const B128 *point = out.unskipped_challenges.data() + (rounds - pr.nr); // the last n - k
		const FSliceMut q = ops::eq_ind_partial_eval(hal, alloc, std::vector<B128>(point, point + pr.nr), false);
		FSliceMut outs = alloc.alloc(t.columns.size() << k);
		std::vector<bn_pe_column> cols;
		std::vector<void *> d_outs;
		std::vector<size_t> on_device;
		for (size_t c = 0; c < t.columns.size(); c++) {
			if (t.n_vars + t.columns[c].tower_level < 7) {
				// less than one 16-byte element: on the host
				std::vector<B128> small(1);
				hal.copy_d2h(FSlice{t.columns[c].d_evals, 1}, small);
				const std::vector<B128> eq = eq_expand(point, pr.nr);
				for (size_t u = 0; u < K; u++) {
					B128 s = B128::ZERO();
					for (size_t j = 0; j < eq.size(); j++) s += eq[j] * packed_element(small, t.columns[c].tower_level, j * K + u);
					projected[first + c][u] = s;
				}
				continue;
			}
			cols.push_back(bn_pe_column{t.columns[c].d_evals, t.columns[c].tower_level, (uint32_t)t.n_vars});
			d_outs.push_back((char *)outs.ptr + (on_device.size() << k) * sizeof(B128));
			on_device.push_back(c);
		}
		if (!cols.empty()) {
			check(bn_partial_eval_high_batch(hal.raw_ctx(), cols.data(), (uint32_t)cols.size(), q.ptr, (uint32_t)pr.nr, d_outs.data()));
			out.phase_calls[Out::Projection] += 2 + (pr.nr ? 1 : 0);
			std::vector<B128> all(on_device.size() << k);
			hal.copy_d2h(FSlice{outs.ptr, all.size()}, all);
			for (size_t i = 0; i < on_device.size(); i++) projected[first + on_device[i]].assign(all.begin() + (i << k), all.begin() + ((i + 1) << k));
		}
	}
	out.phase_ms[Out::Projection] = elapsed_ms(t0);

	// ---- the univariatizing reduction: RegularSumcheckProver, High-to-Low, claims (column i) * (Lagrange multilinear), on the host
	t0 = std::chrono::steady_clock::now();
	std::vector<B128> sums;
	for (const auto &evals : out.final_evals) sums.insert(sums.end(), evals.begin(), evals.end() - 1);
	std::vector<B128> lag = l_sub, reduction_challenges;
	const B128 reduction_batch_coeff = tr.sample(ZerocheckReductionBatchCoeff, 0); // (front_loaded::BatchProver::new, batch_zerocheck.rs:266-267)
	for (size_t r = 0; r < k; r++) {
		const size_t half = (size_t)1 << (k - 1 - r);
		std::vector<B128> l_inf(half);
		for (size_t x = 0; x < half; x++) l_inf[x] = lag[x] + lag[half + x];
		std::vector<B128> coeffs(3, B128::ZERO());
		std::vector<std::array<B128, 3>> per(projected.size()); // every claim's round polynomial: the challenge is drawn after the batched one is written
		B128 scale = reduction_batch_coeff; // the powers of the coefficient, times the coefficient (prove/front_loaded.rs:128-132)
		for (size_t i = 0; i < projected.size(); i++) {
			const std::vector<B128> &a = projected[i];
			B128 y1 = B128::ZERO(), yinf = B128::ZERO();
			for (size_t x = 0; x < half; x++) {
				y1 += a[half + x] * lag[half + x];
				yinf += (a[x] + a[half + x]) * l_inf[x];
			}
			const B128 c0 = sums[i] + y1, c2 = yinf, c1 = y1 + c0 + c2;
			per[i] = {c0, c1, c2};
			coeffs[0] += scale * c0;
			coeffs[1] += scale * c1;
			coeffs[2] += scale * c2;
			scale = scale * reduction_batch_coeff;
		}
		tr.write_scalars(coeffs.data(), 2); // (RoundCoeffs::truncate)
		const B128 z = tr.sample(ZerocheckReductionChallenges, r);
		reduction_challenges.push_back(z);
		for (size_t i = 0; i < projected.size(); i++) {
			std::vector<B128> &a = projected[i];
			sums[i] = per[i][0] + z * (per[i][1] + z * per[i][2]);
			for (size_t x = 0; x < half; x++) a[x] = a[x] + z * (a[x] + a[half + x]);
		}
		for (size_t x = 0; x < half; x++) lag[x] = lag[x] + z * l_inf[x];
		out.reduction_round_coeffs.push_back(coeffs);
	}
	out.skipped_challenges.assign(reduction_challenges.rbegin(), reduction_challenges.rend());
	for (const auto &a : projected) out.reduction_final_evals.push_back(a[0]);
	out.concat_multilinear_evals = out.reduction_final_evals;
	out.reduction_final_evals.push_back(lag[0]);
	tr.write_scalars(out.reduction_final_evals);
	out.phase_ms[Out::Reduction] = elapsed_ms(t0);
	return out;
}
inline ZerocheckBatchOutput zerocheck_batch_prove(ComputeLayer &hal, const std::vector<ZerocheckTable> &tables, size_t skip_rounds, const std::vector<B128> &zerocheck_challenges,
                                                  const std::vector<B128> &batch_coeffs, B128 univariate_challenge, const std::vector<B128> &sumcheck_challenges,
                                                  B128 reduction_batch_coeff, const std::vector<B128> &reduction_challenges, FSliceMut scratch, bool tower = false)
{
	size_t max_n = 0;
	for (const ZerocheckTable &t : tables) max_n = t.n_vars > max_n ? t.n_vars : max_n;
	if (!tables.empty() && skip_rounds <= max_n) { // (otherwise the mirror rejects the call before its first draw)
		const size_t rounds = max_n - skip_rounds;
		if (batch_coeffs.size() != tables.size()) throw Error(Error::InputValidation, "IncorrectNumberOfBatchCoeffs");
		if (zerocheck_challenges.size() != rounds || sumcheck_challenges.size() != rounds || reduction_challenges.size() != skip_rounds)
			throw Error(Error::InputValidation, "zerocheck: max_n - k zerocheck and sumcheck challenges, k reduction challenges");
	}
	ArrayTranscript tr({ArrayTranscript::stream(zerocheck_challenges), ArrayTranscript::stream(batch_coeffs), ArrayTranscript::Stream{&univariate_challenge, 1},
	                    ArrayTranscript::stream(sumcheck_challenges), ArrayTranscript::Stream{&reduction_batch_coeff, 1}, ArrayTranscript::stream(reduction_challenges)});
	return zerocheck_batch_prove(hal, tables, skip_rounds, tr, scratch, tower);
}

} // namespace binius_amd
