// binius_amd/host/witness.hpp -- C++ mirror of the witness-side reading of a MultilinearOracleSet (multilinear.rs of core's oracle module): the
// virtual columns that are pure functions of columns already on the device are built there, instead of being filled on the host and
// uploaded.  The caller lists the columns in oracle-id order; a column is one of
//
//   Given              a device pointer, tower level, n_vars (committed columns, and whatever the caller did upload)
//   Shifted            add_shifted        same level and n_vars as the inner                       BN_DERIVE_SHIFTED
//   Repeating          add_repeating      same level, n_vars = inner + log_count                    BN_DERIVE_REPEATING
//   ZeroPadded         add_zero_padded    same level, n_vars = inner + n_pad_vars                   BN_DERIVE_ZERO_PADDED
//   Packed             add_packed         level = inner + log_degree, n_vars = inner - log_degree   an ALIAS: the inner's pointer, no launch
//   LinearCombination  add_linear_combination[_with_offset]: level = the maximum over its terms' levels and the minimal levels of its
//                      coefficients and offset (multilinear.rs:91-266); all coefficients ONE and every term at that level:
//                      BN_DERIVE_XOR_COMBINATION; otherwise, at level 7, bn_partial_eval_high_lincomb_batch at query_vars = 0 (the
//                      one-element query ONE sits in scratch); otherwise InputValidation
//
// and refers to its inner columns by index, always smaller than its own, as OracleIds are.  witness_build takes these and, through
// bn_generate_columns_batch, the columns that a few integers, one field element or a 0/1 projection determine:
//
//   ProjectedBits      add_projected / add_selected at query values ZERO / ONE: the inner's level, n_vars = inner - query_size
//                                                                                                  BN_GEN_PROJECTED_BITS
//   Constant, StepDown, StepUp, SelectRow, Powers   the transparents of core/src/transparent/ that their parameters determine
//   Incrementing       add_structured(Incrementing)                                                BN_GEN_INCREMENTING
//
// witness_derive keeps rejecting them as unknown kinds.  witness_compute takes all of these and the columns of m3's add_computed
// (m3/src/builder/constraint_system.rs:515-540), each ONE bn_compute_composite with a tower-typed expression (bn_expr_compile_tower):
//
//   Computed           add_computed -> composite_mle: an expression over columns of its n_vars, at the tower level the caller names
//                      (every step's level at most that: the rules of bn_expr_compile_tower)
//   LinearCombination  add_computed -> linear_combination_with_offset, widened: what is neither the XOR form nor a B128 combination
//                      becomes the expression sum of coeff * term + offset, left-deep, at the combination's level (pack_fp / pack_b8:
//                      B1 terms, coefficients in B8 / B32 / B64); a level of 1 or 2 cannot be packed and is InputValidation
//
// witness_compute_batched is witness_compute with the expression columns of a wave in ONE bn_compute_composite over a batch
// (bn_expr_compile_tower_batch): the same columns, the same bytes, one launch per wave that has such columns.
// witness_derive and witness_build keep rejecting those.  NOT taken by any: Projected at other query values
// (bn_partial_eval_high_batch / bn_fold_right are the ops for it), general circuit transparents and StructuredFixedSize, TowerBasis,
// EqIndPartialEval (bn_tensor_expand), ShiftIndPartialEval, DisjointProduct -- the caller derives or uploads those and lists them as
// Given.
//
// Waves: a column's wave is one more than its deepest inner (Given and a generated column without an inner: 0; a Packed alias adds
// nothing).  ONE bn_derive_columns_batch per wave, plus ONE lincomb call per wave that has a B128 combination outside the XOR form,
// plus ONE bn_generate_columns_batch per wave that has generated columns, plus ONE bn_compute_composite per expression column of the
// wave (batching them is left to a later change: n_launches shows the difference).  Columns of less than one 16-byte element are host work
// (their inner down, one element up), as zerocheck.hpp does for its padding; they make no launch.
#pragma once
#include <algorithm>
#include <cstring>

#include "../csrc/compose_tower.hpp"
#include "compute_layer.hpp"

namespace binius_amd {

struct WitnessColumn {
	enum Kind : uint32_t {
		Given = 0, Shifted = 1, Repeating = 2, ZeroPadded = 3, Packed = 4, LinearCombination = 5,
		// witness_build only
		ProjectedBits = 6, Constant = 7, StepDown = 8, StepUp = 9, SelectRow = 10, Incrementing = 11, Powers = 12,
		// witness_compute only
		Computed = 13
	};
	uint32_t kind = Given;
	// Given
	const void *d_evals = nullptr;
	uint32_t tower_level = 0, n_vars = 0; // (LinearCombination: n_vars, which a combination without terms cannot take from them)
	// Shifted / Repeating / ZeroPadded / Packed
	uint32_t inner = 0;
	uint32_t block_size = 0, shift_variant = 0; // Shifted
	uint64_t shift_offset = 0;
	uint32_t log_count = 0;                     // Repeating
	uint32_t n_pad_vars = 0, start_index = 0;   // ZeroPadded
	uint64_t nonzero_index = 0;
	uint32_t log_degree = 0;                    // Packed
	// LinearCombination
	std::vector<uint32_t> terms;
	std::vector<B128> coefficients;
	B128 offset = B128::ZERO();
	// ProjectedBits (inner, start_index above) / StepDown, StepUp, SelectRow (tower_level, n_vars above)
	uint32_t query_size = 0;
	uint64_t query_bits = 0, index = 0;
	B128 value = B128::ZERO(); // Constant: the value; Powers: the base
	// Computed (tower_level, n_vars above): the expression's steps; variable v is column inputs[v]
	std::vector<bn_step> steps;
	std::vector<uint32_t> inputs;
};
struct WitnessResolved {
	const void *ptr = nullptr;
	uint32_t tower_level = 0, n_vars = 0, wave = 0;
};
struct WitnessOutput {
	std::vector<WitnessResolved> columns;
	uint32_t n_waves = 0;    // the largest wave of a column
	uint32_t n_launches = 0; // bn_derive_columns_batch, lincomb, bn_generate_columns_batch and bn_compute_composite calls made
};

inline size_t witness_column_elems(size_t n_vars, uint32_t level) { return n_vars + level <= 7 ? 1 : (size_t)1 << (n_vars + level - 7); }
// binary_tower_level() of a field element: the smallest level whose field holds it
inline uint32_t witness_min_level(B128 c)
{
	if (c.hi) return 7;
	uint32_t level = 0;
	while (level < 6 && (c.lo >> (1u << level))) level++;
	return level;
}

// How a column is made: by the derive op, by the lincomb op, by the generate op, by bn_compute_composite with a tower-typed
// expression, on the host, or not at all (Given, Packed)
enum class WitnessRoute { None, Derive, Lincomb, Host, Generate, Compose };
struct WitnessShape {
	uint32_t tower_level = 0, n_vars = 0, wave = 0;
	WitnessRoute route = WitnessRoute::None;
	bool expr = false; // made from witness_expr (a Compose column, or one below one element that the host evaluates)
};

// The expression of a column that goes to bn_compute_composite: a Computed column's own; a combination's sum of coeff * term + offset,
// left-deep (a coefficient ONE costs no product), variable t its term t
struct WitnessExpr {
	std::vector<bn_step> steps;
	std::vector<uint32_t> inputs;
};
inline WitnessExpr witness_expr(const WitnessColumn &c)
{
	if (c.kind == WitnessColumn::Computed) return WitnessExpr{c.steps, c.inputs};
	WitnessExpr e;
	e.inputs = c.terms;
	auto push = [&](uint32_t kind, uint32_t a, uint64_t b, B128 cst) {
		bn_step st{};
		st.kind = kind;
		st.a = a;
		st.b = b;
		st.cst = cst.raw();
		e.steps.push_back(st);
		return (uint32_t)e.steps.size() - 1;
	};
	uint32_t acc = 0;
	for (size_t t = 0; t < c.terms.size(); t++) {
		uint32_t term = push(BN_STEP_VAR, (uint32_t)t, 0, B128::ZERO());
		if (c.coefficients[t] != B128::ONE()) term = push(BN_STEP_MUL, term, push(BN_STEP_CONST, 0, 0, c.coefficients[t]), B128::ZERO());
		acc = t ? push(BN_STEP_ADD, acc, term, B128::ZERO()) : term;
	}
	if (c.terms.empty() || c.offset != B128::ZERO()) {
		const uint32_t off = push(BN_STEP_CONST, 0, 0, c.offset);
		if (!c.terms.empty()) push(BN_STEP_ADD, acc, off, B128::ZERO());
	}
	return e;
}

// Levels, sizes, waves and routes of every column; every rule of the header is checked here, before the first device call.
// generate: witness_build's kinds are taken (otherwise they are unknown kinds); compute: witness_compute's as well.
inline std::vector<WitnessShape> witness_shapes(const std::vector<WitnessColumn> &cols, bool generate = false, bool compute = false)
{
	auto bad = [](const char *msg) { return Error(Error::InputValidation, msg); };
	std::vector<WitnessShape> sh(cols.size());
	// an expression column: the rules of bn_expr_compile_tower over the levels of its inputs, checked by its compiler
	auto check_expr = [&](const WitnessColumn &c, uint32_t out_level, size_t i) {
		const WitnessExpr e = witness_expr(c);
		std::vector<uint32_t> levels;
		for (const uint32_t v : e.inputs) {
			if (v >= i) throw bad("witness: an inner index is smaller than the column's own");
			if (sh[v].n_vars != c.n_vars) throw bad("witness: the inputs of an expression column have its n_vars");
			levels.push_back(sh[v].tower_level);
		}
		bn::ct_program prog;
		const uint32_t none = 0;
		const char *why = bn::ct_compile(e.steps.data(), e.steps.size(), levels.empty() ? &none : levels.data(), (uint32_t)levels.size(), out_level, prog);
		if (why) throw Error(Error::InputValidation, std::string("witness: expression column: ") + why);
	};
	for (size_t i = 0; i < cols.size(); i++) {
		const WitnessColumn &c = cols[i];
		WitnessShape &s = sh[i];
		if (c.kind > WitnessColumn::LinearCombination && !generate) throw bad("witness: unknown column kind");
		if (c.kind > WitnessColumn::Powers && !compute) throw bad("witness: unknown column kind");
		if (((c.kind >= WitnessColumn::Shifted && c.kind <= WitnessColumn::Packed) || c.kind == WitnessColumn::ProjectedBits) && c.inner >= i)
			throw bad("witness: an inner index is smaller than the column's own");
		const bool in_level = c.tower_level >= 7 || (c.value.hi == 0 && (c.tower_level == 6 || c.value.lo < ((uint64_t)1 << (1u << c.tower_level))));
		if (c.kind >= WitnessColumn::Constant && c.kind <= WitnessColumn::Powers) {
			if (c.tower_level > 7 || c.tower_level == 1 || c.tower_level == 2) throw bad("witness: unsupported tower level");
			if (c.n_vars > BN_PE_MAX_VARS) throw bad("witness: a column has at most 2^40 values");
			s = WitnessShape{c.tower_level, c.n_vars, 0, WitnessRoute::Generate};
		}
		switch (c.kind) {
		case WitnessColumn::Given:
			if (!c.d_evals) throw bad("witness: null given column");
			if (c.tower_level > 7 || c.tower_level == 1 || c.tower_level == 2) throw bad("witness: unsupported tower level");
			s = WitnessShape{c.tower_level, c.n_vars, 0, WitnessRoute::None};
			break;
		case WitnessColumn::Shifted:
			s = WitnessShape{sh[c.inner].tower_level, sh[c.inner].n_vars, sh[c.inner].wave + 1, WitnessRoute::Derive};
			if (c.shift_variant > BN_SHIFT_LOGICAL_RIGHT) throw bad("witness: unknown shift variant");
			if (c.block_size > s.n_vars || c.shift_offset == 0 || c.block_size > BN_PE_MAX_VARS || c.shift_offset >= ((uint64_t)1 << c.block_size))
				throw bad("witness: Shifted needs block_size <= n_vars and 1 <= shift_offset < 2^block_size");
			break;
		case WitnessColumn::Repeating:
			if (c.log_count > BN_PE_MAX_VARS) throw bad("witness: log_count out of range");
			s = WitnessShape{sh[c.inner].tower_level, sh[c.inner].n_vars + c.log_count, sh[c.inner].wave + 1, WitnessRoute::Derive};
			break;
		case WitnessColumn::ZeroPadded:
			if (c.n_pad_vars > BN_PE_MAX_VARS) throw bad("witness: n_pad_vars out of range");
			s = WitnessShape{sh[c.inner].tower_level, sh[c.inner].n_vars + c.n_pad_vars, sh[c.inner].wave + 1, WitnessRoute::Derive};
			if (c.start_index > sh[c.inner].n_vars) throw bad("IncorrectStartIndex: start_index > inner n_vars");
			if (c.nonzero_index >= ((uint64_t)1 << c.n_pad_vars)) throw bad("IncorrectNonZeroIndex: nonzero_index >= 2^n_pad_vars");
			break;
		case WitnessColumn::Packed:
			if (c.log_degree > sh[c.inner].n_vars || sh[c.inner].tower_level + c.log_degree > 7) throw bad("witness: Packed leaves the tower or the column");
			s = WitnessShape{sh[c.inner].tower_level + c.log_degree, sh[c.inner].n_vars - c.log_degree, sh[c.inner].wave, WitnessRoute::None};
			if (s.tower_level == 1 || s.tower_level == 2) throw bad("witness: unsupported tower level");
			break;
		case WitnessColumn::LinearCombination: {
			if (c.terms.size() != c.coefficients.size()) throw bad("witness: one coefficient per term");
			if (c.terms.size() > BN_PEL_MAX_TERMS) throw bad("witness: too many terms in a combination");
			uint32_t level = witness_min_level(c.offset), wave = 0;
			uint32_t raw_level = 0;
			bool unit = true;
			for (size_t t = 0; t < c.terms.size(); t++) {
				if (c.terms[t] >= i) throw bad("witness: an inner index is smaller than the column's own");
				if (sh[c.terms[t]].n_vars != c.n_vars) throw bad("witness: the terms of a combination have its n_vars");
				level = std::max({level, sh[c.terms[t]].tower_level, witness_min_level(c.coefficients[t])});
				wave = std::max(wave, sh[c.terms[t]].wave);
				unit = unit && c.coefficients[t] == B128::ONE();
			}
			raw_level = level;
			if (level == 1 || level == 2) level = 3; // (the packed levels of this backend: a B2 / B4 constant lives in a B8 column)
			for (const uint32_t t : c.terms) unit = unit && sh[t].tower_level == level;
			s = WitnessShape{level, c.n_vars, wave + 1, unit ? WitnessRoute::Derive : WitnessRoute::Lincomb};
			if (!unit && level != 7 && compute) {
				// the reference's level (multilinear.rs:91-266), as a tower-typed expression
				if (raw_level == 1 || raw_level == 2) throw bad("witness: a combination of tower level 1 or 2 cannot be packed");
				check_expr(c, raw_level, i);
				s = WitnessShape{raw_level, c.n_vars, wave + 1, WitnessRoute::Compose, true};
				break;
			}
			if (!unit && level != 7)
				throw bad("witness: a combination is either all ONE coefficients over terms of its own level or a B128 one (Projected, Composite, transparent and "
				          "structured columns are not taken either: list them as Given)");
			break;
		}
		case WitnessColumn::ProjectedBits:
			if (c.query_size < 1 || c.query_size > sh[c.inner].n_vars || c.start_index > sh[c.inner].n_vars - c.query_size)
				throw bad("witness: ProjectedBits needs query_size >= 1 and start_index + query_size <= inner n_vars");
			if (c.query_bits >= ((uint64_t)1 << c.query_size)) throw bad("witness: query_bits >= 2^query_size");
			s = WitnessShape{sh[c.inner].tower_level, sh[c.inner].n_vars - c.query_size, sh[c.inner].wave + 1, WitnessRoute::Generate};
			break;
		case WitnessColumn::Constant:
			if (!in_level) throw bad("witness: the value of a Constant is a value of its tower level");
			break;
		case WitnessColumn::StepDown:
		case WitnessColumn::StepUp:
			if (c.tower_level != 0) throw bad("witness: a step column is a B1 column");
			if (c.index > ((uint64_t)1 << c.n_vars)) throw bad("witness: a step's index is at most 2^n_vars");
			break;
		case WitnessColumn::SelectRow:
			if (c.tower_level != 0) throw bad("witness: a select-row column is a B1 column");
			if (c.index >= ((uint64_t)1 << c.n_vars)) throw bad("witness: a selected row is below 2^n_vars");
			break;
		case WitnessColumn::Incrementing:
			if (c.n_vars > (1u << c.tower_level)) throw bad("witness: an incrementing column has n_vars <= 2^tower_level");
			break;
		case WitnessColumn::Powers:
			if (c.tower_level < 3) throw bad("witness: a column of powers has tower level 3 .. 7");
			if (!in_level) throw bad("witness: the base of Powers is a value of its tower level");
			break;
		case WitnessColumn::Computed: {
			if (c.n_vars > BN_PE_MAX_VARS) throw bad("witness: a column has at most 2^40 values");
			check_expr(c, c.tower_level, i);
			uint32_t wave = 0;
			for (const uint32_t v : c.inputs) wave = std::max(wave, sh[v].wave);
			s = WitnessShape{c.tower_level, c.n_vars, wave + 1, WitnessRoute::Compose, true};
			break;
		}
		default:
			throw bad("witness: unknown column kind");
		}
		if (s.n_vars > BN_PE_MAX_VARS) throw bad("witness: a column has at most 2^40 values");
		if ((s.route == WitnessRoute::Derive || s.route == WitnessRoute::Generate || s.route == WitnessRoute::Compose) && s.n_vars + s.tower_level < 7)
			s.route = WitnessRoute::Host;
	}
	return sh;
}

// Exact: one element for the query ONE when a combination goes to the lincomb op, then every derived column at its packed size.
inline size_t witness_derive_scratch_elems(const std::vector<WitnessColumn> &cols, bool generate = false, bool compute = false)
{
	const std::vector<WitnessShape> sh = witness_shapes(cols, generate, compute);
	size_t total = 0;
	bool one = false;
	for (const WitnessShape &s : sh) {
		if (s.route == WitnessRoute::None) continue;
		one = one || s.route == WitnessRoute::Lincomb;
		total += witness_column_elems(s.n_vars, s.tower_level);
	}
	return total + (one ? 1 : 0);
}

namespace witness_detail {
// value i (2^level <= 64 bits) of a packed column of at most 128 bits
inline uint64_t get(const B128 &e, uint32_t level, size_t i)
{
	const size_t w = (size_t)1 << level, bit = i * w;
	const uint64_t word = bit < 64 ? e.lo : e.hi;
	return w == 64 ? word : (word >> (bit & 63)) & (((uint64_t)1 << w) - 1);
}
// value i (2^level <= 64 bits) of a packed column of any number of elements
inline uint64_t get(const std::vector<B128> &col, uint32_t level, size_t i) { return get(col[(i << level) >> 7], level, i & ((128u >> level) - 1)); }
inline void put(B128 &e, uint32_t level, size_t i, uint64_t v)
{
	const size_t bit = (i << level);
	(bit < 64 ? e.lo : e.hi) |= v << (bit & 63);
}
} // namespace witness_detail

// A generated column of less than one element, value by value (the definitions bn_generate_columns_batch cites); inner: the whole inner
// column of a projection
inline B128 witness_small_generated(const WitnessColumn &c, const WitnessShape &s, const std::vector<B128> &inner)
{
	const uint32_t l = s.tower_level;
	const size_t n = (size_t)1 << s.n_vars;
	B128 out = B128::ZERO(), power = B128::ONE();
	for (size_t i = 0; i < n; i++) {
		uint64_t v = 0;
		switch (c.kind) {
		case WitnessColumn::ProjectedBits: {
			const size_t run = (size_t)1 << c.start_index, lo = i & (run - 1), hi = i >> c.start_index;
			v = witness_detail::get(inner, l, lo + ((size_t)c.query_bits << c.start_index) + (hi << (c.start_index + c.query_size)));
			break;
		}
		case WitnessColumn::Constant: v = c.value.lo; break;
		case WitnessColumn::StepDown: v = i < c.index; break;
		case WitnessColumn::StepUp: v = i >= c.index; break;
		case WitnessColumn::SelectRow: v = i == c.index; break;
		case WitnessColumn::Incrementing: v = i; break;
		default: // Powers
			v = power.lo;
			power = power * c.value;
			break;
		}
		witness_detail::put(out, l, i, v);
	}
	return out;
}

// A column of less than one element, value by value (validate.rs:151-279, fold.rs:52-75) from its inner columns' single elements
inline B128 witness_small_column(const WitnessColumn &c, const WitnessShape &s, const std::vector<WitnessShape> &sh, const std::vector<B128> &inners)
{
	using witness_detail::get;
	using witness_detail::put;
	const uint32_t l = s.tower_level;
	const size_t n = (size_t)1 << s.n_vars;
	B128 out = B128::ZERO();
	for (size_t i = 0; i < n; i++) {
		uint64_t v = 0;
		switch (c.kind) {
		case WitnessColumn::Shifted: {
			const size_t B = (size_t)1 << c.block_size, o = i & (B - 1), blk = i - o, sft = (size_t)c.shift_offset;
			if (c.shift_variant == BN_SHIFT_CIRCULAR_LEFT)
				v = get(inners[0], l, blk + ((o + B - sft) & (B - 1)));
			else if (c.shift_variant == BN_SHIFT_LOGICAL_LEFT)
				v = o >= sft ? get(inners[0], l, blk + o - sft) : 0;
			else
				v = o + sft < B ? get(inners[0], l, blk + o + sft) : 0;
			break;
		}
		case WitnessColumn::Repeating:
			v = get(inners[0], l, i & (((size_t)1 << sh[c.inner].n_vars) - 1));
			break;
		case WitnessColumn::ZeroPadded: {
			const size_t run = (size_t)1 << c.start_index, period = run << c.n_pad_vars, col = i & (period - 1), row = i / period, z = (size_t)c.nonzero_index * run;
			v = col >= z && col < z + run ? get(inners[0], l, row * run + col - z) : 0;
			break;
		}
		default:
			v = c.offset.lo;
			for (const B128 &t : inners) v ^= get(t, l, i);
			break;
		}
		put(out, l, i, v);
	}
	return out;
}

// An expression column of less than one element, value by value in B128 (bn_scalar_mul) from its inputs' single elements
inline B128 witness_small_expr(const WitnessExpr &e, const WitnessShape &s, const std::vector<uint32_t> &in_levels, const std::vector<B128> &inners)
{
	B128 out = B128::ZERO();
	std::vector<B128> val(e.steps.size());
	for (size_t i = 0; i < ((size_t)1 << s.n_vars); i++) {
		for (size_t k = 0; k < e.steps.size(); k++) {
			const bn_step &st = e.steps[k];
			switch (st.kind) {
			case BN_STEP_VAR: val[k] = B128(witness_detail::get(inners[st.a], in_levels[st.a], i)); break;
			case BN_STEP_CONST: val[k] = B128(st.cst.lo, st.cst.hi); break;
			case BN_STEP_ADD: val[k] = val[st.a] + val[st.b]; break;
			case BN_STEP_MUL: val[k] = val[st.a] * val[st.b]; break;
			default: { // POW
				B128 r = B128::ONE();
				for (int b = 63; b >= 0; b--) {
					r = r * r;
					if ((st.b >> b) & 1) r = r * val[st.a];
				}
				val[k] = r;
				break;
			}
			}
		}
		witness_detail::put(out, s.tower_level, i, val.back().lo); // (below one element: the level is at most 6, and subfields are closed)
	}
	return out;
}

// The expression columns `composed` of one wave in ONE bn_compute_composite: every distinct (steps, input levels, output level) is
// compiled once, the batch's arena is the plan's scratch and a job's out_offset its column's place in it; a job's rows are its inputs,
// one after the other in the call's row list.  The handles live for the call alone.
inline void witness_compose_wave(ComputeLayer &hal, const std::vector<WitnessColumn> &cols, const std::vector<WitnessShape> &sh, const WitnessOutput &out,
                                 const std::vector<size_t> &composed, FSliceMut scratch)
{
	struct Compiled {
		WitnessExpr e;
		std::vector<uint32_t> levels;
		uint32_t out_level;
	};
	auto same_steps = [](const std::vector<bn_step> &x, const std::vector<bn_step> &y) {
		if (x.size() != y.size()) return false;
		for (size_t k = 0; k < x.size(); k++)
			if (x[k].kind != y[k].kind || x[k].a != y[k].a || x[k].b != y[k].b || x[k].cst.lo != y[k].cst.lo || x[k].cst.hi != y[k].cst.hi) return false;
		return true;
	};
	std::vector<Compiled> distinct;
	std::vector<bn_expr *> handles;
	std::vector<bn_compose_job> jobs;
	std::vector<const void *> rows;
	auto free_all = [&]() {
		for (bn_expr *h : handles) bn_expr_free(h);
		handles.clear();
	};
	try {
		for (const size_t i : composed) {
			Compiled c{witness_expr(cols[i]), {}, sh[i].tower_level};
			for (const uint32_t v : c.e.inputs) c.levels.push_back(sh[v].tower_level);
			uint32_t k = 0;
			while (k < distinct.size() && !(distinct[k].out_level == c.out_level && distinct[k].levels == c.levels && same_steps(distinct[k].e.steps, c.e.steps))) k++;
			if (k == distinct.size()) {
				const uint32_t none = 0;
				bn_expr *h = nullptr;
				check(bn_expr_compile_tower(hal.raw_ctx(), c.e.steps.data(), c.e.steps.size(), c.levels.empty() ? &none : c.levels.data(), (uint32_t)c.levels.size(), c.out_level, &h));
				handles.push_back(h);
				distinct.push_back(c);
			}
			bn_compose_job jb{};
			jb.expr = k;
			jb.first_row = (uint32_t)rows.size();
			jb.n_vars = sh[i].n_vars;
			jb.out_offset = (uint64_t)((const char *)out.columns[i].ptr - (const char *)scratch.ptr) / 16;
			jobs.push_back(jb);
			for (const uint32_t v : c.e.inputs) rows.push_back(out.columns[v].ptr);
		}
		std::vector<uint32_t> desc;
		std::vector<uint64_t> offsets;
		for (const bn_compose_job &j : jobs) {
			desc.insert(desc.end(), {j.expr, j.first_row, j.n_vars, j.reserved});
			offsets.push_back(j.out_offset);
		}
		bn_expr *batch = nullptr;
		check(bn_expr_compile_tower_batch(hal.raw_ctx(), handles.data(), (uint32_t)handles.size(), desc.data(), offsets.data(), (uint32_t)jobs.size(), &batch));
		free_all(); // (the batch holds copies of the programs)
		const void *no_row = nullptr;
		const int rc = bn_compute_composite(hal.raw_ctx(), rows.empty() ? &no_row : rows.data(), (uint32_t)rows.size(), scratch.len_, scratch.ptr, scratch.len_, batch);
		bn_expr_free(batch);
		check(rc);
	} catch (...) {
		free_all();
		throw;
	}
}

// batched: the expression columns of a wave go through witness_compose_wave, one launch, instead of one bn_compute_composite each
inline WitnessOutput witness_derive(ComputeLayer &hal, const std::vector<WitnessColumn> &cols, FSliceMut scratch, bool generate = false, bool compute = false,
                                    bool batched = false)
{
	const std::vector<WitnessShape> sh = witness_shapes(cols, generate, compute);
	if (scratch.len_ < witness_derive_scratch_elems(cols, generate, compute)) throw Error(Error::InputValidation, "scratch holds fewer than witness_derive_scratch_elems elements");
	DeviceBumpAllocator alloc(scratch);
	WitnessOutput out;
	out.columns.resize(cols.size());
	FSliceMut d_one;
	if (std::any_of(sh.begin(), sh.end(), [](const WitnessShape &s) { return s.route == WitnessRoute::Lincomb; })) {
		d_one = alloc.alloc(1);
		hal.fill(d_one, B128::ONE());
	}
	for (size_t i = 0; i < cols.size(); i++) {
		WitnessResolved &r = out.columns[i];
		r.tower_level = sh[i].tower_level;
		r.n_vars = sh[i].n_vars;
		r.wave = sh[i].wave;
		out.n_waves = std::max(out.n_waves, r.wave);
		if (cols[i].kind == WitnessColumn::Given)
			r.ptr = cols[i].d_evals;
		else if (cols[i].kind == WitnessColumn::Packed)
			r.ptr = out.columns[cols[i].inner].ptr; // (inner < i: resolved, and a derived inner already has its place in scratch)
		else
			r.ptr = alloc.alloc(witness_column_elems(r.n_vars, r.tower_level)).ptr;
	}
	for (uint32_t wave = 0; wave <= out.n_waves; wave++) { // (wave 0 has work only where a generated column has no inner)
		std::vector<bn_derive_job> jobs;
		std::vector<bn_generate_job> gen_jobs;
		std::vector<const void *> terms;
		std::vector<bn_pel_job> pel_jobs;
		std::vector<bn_pel_term> pel_terms;
		std::vector<void *> pel_outs;
		std::vector<size_t> on_host, composed;
		for (size_t i = 0; i < cols.size(); i++) {
			if (sh[i].wave != wave || sh[i].route == WitnessRoute::None) continue;
			const WitnessColumn &c = cols[i];
			if (sh[i].route == WitnessRoute::Host) {
				on_host.push_back(i);
				continue;
			}
			if (sh[i].route == WitnessRoute::Compose) {
				composed.push_back(i);
				continue;
			}
			if (sh[i].route == WitnessRoute::Generate) {
				bn_generate_job jb{};
				static_assert(BN_GEN_PROJECTED_BITS == 0 && BN_GEN_POWERS == WitnessColumn::Powers - WitnessColumn::ProjectedBits, "BN_GEN_* in WitnessColumn's order");
				jb.kind = c.kind - WitnessColumn::ProjectedBits;
				jb.tower_level = sh[i].tower_level;
				jb.n_vars = sh[i].n_vars;
				jb.d_out = const_cast<void *>(out.columns[i].ptr);
				if (c.kind == WitnessColumn::ProjectedBits) {
					jb.d_inner = out.columns[c.inner].ptr;
					jb.start_index = c.start_index;
					jb.query_size = c.query_size;
					jb.query_bits = c.query_bits;
				}
				jb.index = c.index;
				jb.value = c.value.raw();
				gen_jobs.push_back(jb);
				continue;
			}
			if (sh[i].route == WitnessRoute::Lincomb) {
				pel_jobs.push_back(bn_pel_job{sh[i].n_vars, (uint32_t)pel_terms.size(), (uint32_t)c.terms.size(), 0, c.offset.raw()});
				for (size_t t = 0; t < c.terms.size(); t++)
					pel_terms.push_back(bn_pel_term{out.columns[c.terms[t]].ptr, sh[c.terms[t]].tower_level, 0, c.coefficients[t].raw()});
				pel_outs.push_back(const_cast<void *>(out.columns[i].ptr));
				continue;
			}
			bn_derive_job jb{};
			jb.tower_level = sh[i].tower_level;
			jb.n_vars = sh[i].n_vars;
			jb.d_out = const_cast<void *>(out.columns[i].ptr);
			if (c.kind != WitnessColumn::LinearCombination) {
				jb.d_inner = out.columns[c.inner].ptr;
				jb.inner_n_vars = sh[c.inner].n_vars;
			}
			switch (c.kind) {
			case WitnessColumn::Shifted:
				jb.kind = BN_DERIVE_SHIFTED;
				jb.block_size = c.block_size;
				jb.shift_variant = c.shift_variant;
				jb.shift_offset = c.shift_offset;
				break;
			case WitnessColumn::Repeating:
				jb.kind = BN_DERIVE_REPEATING;
				break;
			case WitnessColumn::ZeroPadded:
				jb.kind = BN_DERIVE_ZERO_PADDED;
				jb.start_index = c.start_index;
				jb.nonzero_index = c.nonzero_index;
				break;
			default:
				jb.kind = BN_DERIVE_XOR_COMBINATION;
				jb.first_term = (uint32_t)terms.size();
				jb.n_terms = (uint32_t)c.terms.size();
				jb.offset = c.offset.raw();
				for (const uint32_t t : c.terms) terms.push_back(out.columns[t].ptr);
				break;
			}
			jobs.push_back(jb);
		}
		if (!jobs.empty()) {
			check(bn_derive_columns_batch(hal.raw_ctx(), jobs.data(), (uint32_t)jobs.size(), terms.data(), (uint32_t)terms.size()));
			out.n_launches++;
		}
		if (!pel_jobs.empty()) {
			check(bn_partial_eval_high_lincomb_batch(hal.raw_ctx(), pel_jobs.data(), (uint32_t)pel_jobs.size(), pel_terms.data(), (uint32_t)pel_terms.size(), d_one.ptr, 0,
			                                         pel_outs.data()));
			out.n_launches++;
		}
		if (!gen_jobs.empty()) {
			check(bn_generate_columns_batch(hal.raw_ctx(), gen_jobs.data(), (uint32_t)gen_jobs.size()));
			out.n_launches++;
		}
		if (batched && !composed.empty()) {
			witness_compose_wave(hal, cols, sh, out, composed, scratch);
			out.n_launches++;
			composed.clear();
		}
		for (const size_t i : composed) { // one bn_compute_composite per expression column
			const WitnessExpr e = witness_expr(cols[i]);
			std::vector<uint32_t> levels;
			std::vector<const void *> rows;
			for (const uint32_t v : e.inputs) {
				levels.push_back(sh[v].tower_level);
				rows.push_back(out.columns[v].ptr);
			}
			const uint32_t none = 0;
			bn_expr *h = nullptr;
			check(bn_expr_compile_tower(hal.raw_ctx(), e.steps.data(), e.steps.size(), levels.empty() ? &none : levels.data(), (uint32_t)levels.size(), sh[i].tower_level, &h));
			const void *no_row = nullptr;
			const uint64_t n_values = (uint64_t)1 << sh[i].n_vars;
			const int rc = bn_compute_composite(hal.raw_ctx(), rows.empty() ? &no_row : rows.data(), (uint32_t)rows.size(), n_values, const_cast<void *>(out.columns[i].ptr),
			                                    n_values, h);
			bn_expr_free(h);
			check(rc);
			out.n_launches++;
		}
		for (const size_t i : on_host) {
			const WitnessColumn &c = cols[i];
			if (sh[i].expr) {
				const WitnessExpr e = witness_expr(c);
				std::vector<uint32_t> levels;
				std::vector<B128> inners(e.inputs.size()), one(1);
				for (size_t t = 0; t < e.inputs.size(); t++) {
					levels.push_back(sh[e.inputs[t]].tower_level);
					hal.copy_d2h(FSlice{out.columns[e.inputs[t]].ptr, 1}, one);
					inners[t] = one[0];
				}
				one[0] = witness_small_expr(e, sh[i], levels, inners);
				FSliceMut dst{const_cast<void *>(out.columns[i].ptr), 1};
				hal.copy_h2d(one, dst);
				continue;
			}
			if (c.kind >= WitnessColumn::ProjectedBits) {
				std::vector<B128> inner, one(1);
				if (c.kind == WitnessColumn::ProjectedBits) {
					inner.resize(witness_column_elems(sh[c.inner].n_vars, sh[c.inner].tower_level));
					hal.copy_d2h(FSlice{out.columns[c.inner].ptr, inner.size()}, inner);
				}
				one[0] = witness_small_generated(c, sh[i], inner);
				FSliceMut dst{const_cast<void *>(out.columns[i].ptr), 1};
				hal.copy_h2d(one, dst);
				continue;
			}
			std::vector<uint32_t> ids = c.kind == WitnessColumn::LinearCombination ? c.terms : std::vector<uint32_t>{c.inner};
			std::vector<B128> inners(ids.size()), one(1);
			for (size_t t = 0; t < ids.size(); t++) {
				hal.copy_d2h(FSlice{out.columns[ids[t]].ptr, 1}, one);
				inners[t] = one[0];
			}
			one[0] = witness_small_column(c, sh[i], sh, inners);
			FSliceMut dst{const_cast<void *>(out.columns[i].ptr), 1};
			hal.copy_h2d(one, dst);
		}
	}
	return out;
}

// witness_derive with the generated kinds taken (the header)
inline size_t witness_build_scratch_elems(const std::vector<WitnessColumn> &cols) { return witness_derive_scratch_elems(cols, true); }
inline WitnessOutput witness_build(ComputeLayer &hal, const std::vector<WitnessColumn> &cols, FSliceMut scratch) { return witness_derive(hal, cols, scratch, true); }
// witness_build with the expression columns taken as well (the header)
inline size_t witness_compute_scratch_elems(const std::vector<WitnessColumn> &cols) { return witness_derive_scratch_elems(cols, true, true); }
inline WitnessOutput witness_compute(ComputeLayer &hal, const std::vector<WitnessColumn> &cols, FSliceMut scratch) { return witness_derive(hal, cols, scratch, true, true); }
// witness_compute with the expression columns of a wave in one launch (bn_expr_compile_tower_batch); witness_compute_scratch_elems serves both
inline WitnessOutput witness_compute_batched(ComputeLayer &hal, const std::vector<WitnessColumn> &cols, FSliceMut scratch)
{
	return witness_derive(hal, cols, scratch, true, true, true);
}

} // namespace binius_amd
