// binius_amd/csrc/compose_tower.hpp -- tower-typed expressions (bn_expr_compile_tower): the compiler from a step list to the program
// of kernels_compose_tower.hip, and the arithmetic on packed subfield elements that the kernel runs.  Plain C++ with the BN_HD
// markers of gf128.hpp: the same functions run in the kernel, in the host path of a caller and in a stand-alone program on the CPU
// (tests/cpp/compose_tower_check.cpp, which is also the target of a host sanitizer build).
//
// The values of an input at level l are zero-extended into the 2^L-bit places of the output level L (the tower embedding is the
// identity on the low bits, binary_field.rs:361-412), a 16-byte element then holds 2^(7 - L) values and every operation works on all
// of them at once: ADD is XOR; multiplication by X_k (gf128.hpp mulx<k>) acts on every 2^(k+1)-bit limb alone, so for k < L it never
// leaves a value's place, and a product is the bilinear walk of mul_walk with the bit of the NARROWER operand spread over its place
// as a mask.  Subfields are closed, so no place ever holds a value above its operands' levels.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/binius_amd.h"
#include "gf128.hpp"

namespace bn {

// an operand of an op: a slot, an input column or an entry of the constant table
constexpr uint32_t kCtSlot = 0u << 30, kCtInput = 1u << 30, kCtConst = 2u << 30, kCtTagMask = 3u << 30, kCtIdxMask = ~kCtTagMask;
struct ct_op {
	uint32_t kind;  // BN_STEP_ADD / MUL / POW
	uint32_t dst;   // slot
	uint32_t a;     // MUL: the operand of the higher level; POW: the base
	uint32_t b;     // MUL: the operand of the lower level, whose bits are walked
	uint64_t exp;   // POW
	uint32_t level; // MUL: the lower level; POW: the base's level
	uint32_t reserved;
};
static_assert(sizeof(ct_op) == 32, "ct_op is read by the device in this layout");

struct ct_program {
	std::vector<ct_op> ops;
	std::vector<f128> consts; // every constant at every value's place of an output element
	std::vector<uint32_t> input_levels;
	uint32_t out_level = 0;
	uint32_t n_slots = 0; // the most slots live at once
	uint32_t result = 0;  // operand that holds the value of the expression
};

// A workgroup of the kernel takes kComposeUnitElems contiguous output elements, a thread `compose_tower_per_thread` of them at a time:
// the LDS of a slot is 16 B x 256 threads per element, so up to 4, 8 or 16 live slots fit 64 KiB at 4, 2 or 1 elements per thread.
constexpr uint32_t kComposeUnitElems = 1024;
BN_HD inline uint32_t compose_tower_per_thread(uint32_t n_slots) { return n_slots <= 4 ? 4 : n_slots <= 8 ? 2 : 1; }
BN_HD inline uint32_t compose_tower_lds_bytes(uint32_t n_slots) { return (n_slots ? n_slots : 1) * compose_tower_per_thread(n_slots) * 16 * 256; }

// the smallest l with c < 2^(2^l)
inline uint32_t ct_const_level(uint64_t lo, uint64_t hi)
{
	if (hi) return 7;
	uint32_t l = 0;
	while (l < 6 && (lo >> (1u << l)) != 0) l++;
	return l;
}

// a value below 2^(2^L) at every place of an element of level L
BN_HD inline f128 ct_broadcast(f128 c, uint32_t L)
{
	if (L == 7) return c;
	if (L == 0) return (c.lo & 1) ? f128{~0ull, ~0ull} : f128{0, 0};
	uint64_t w = c.lo;
	for (uint32_t sh = 1u << L; sh < 64; sh <<= 1) w |= w << sh;
	return f128{w, w};
}

// Compiles `steps` (topological order, the last one is the result).  Returns nullptr and fills `p`, or the reason of the rejection;
// nothing is kept of a rejected expression.
inline const char *ct_compile(const bn_step *steps, uint64_t n_steps, const uint32_t *input_levels, uint32_t n_inputs, uint32_t out_level, ct_program &p)
{
	auto packable = [](uint32_t l) { return l == 0 || (l >= 3 && l <= 7); };
	if (!steps || (n_inputs && !input_levels)) return "null argument";
	if (n_steps == 0 || n_steps > BN_TOWER_EXPR_MAX_STEPS) return "number of steps is 0 or above BN_TOWER_EXPR_MAX_STEPS";
	if (n_inputs > BN_TOWER_EXPR_MAX_INPUTS) return "more inputs than BN_TOWER_EXPR_MAX_INPUTS";
	if (!packable(out_level)) return "the output's tower level is 1, 2 or above 7";
	for (uint32_t v = 0; v < n_inputs; v++)
		if (!packable(input_levels[v])) return "an input's tower level is 1, 2 or above 7";
	const uint32_t n = (uint32_t)n_steps;
	std::vector<uint32_t> level(n);
	for (uint32_t s = 0; s < n; s++) {
		const bn_step &st = steps[s];
		switch (st.kind) {
		case BN_STEP_VAR:
			if (st.a >= n_inputs) return "a variable index is not below the number of inputs";
			level[s] = input_levels[st.a];
			break;
		case BN_STEP_CONST: level[s] = ct_const_level(st.cst.lo, st.cst.hi); break;
		case BN_STEP_ADD:
		case BN_STEP_MUL:
			if (st.a >= s || st.b >= s) return "circuit step refers to a later step";
			level[s] = level[st.a] > level[(uint32_t)st.b] ? level[st.a] : level[(uint32_t)st.b];
			break;
		case BN_STEP_POW:
			if (st.a >= s) return "circuit step refers to a later step";
			level[s] = level[st.a];
			break;
		default: return "unknown circuit step kind";
		}
		if (level[s] > out_level) return "a step's tower level is above the output's";
	}
	// steps that feed the result, and the last step that reads each of them
	std::vector<uint32_t> last_use(n, 0);
	std::vector<char> live(n, 0);
	live[n - 1] = 1;
	last_use[n - 1] = n; // (the result is read by the store, after every step)
	for (uint32_t s = n; s-- > 0;) {
		if (!live[s]) continue;
		const bn_step &st = steps[s];
		auto use = [&](uint32_t o) {
			live[o] = 1;
			if (last_use[o] < s) last_use[o] = s;
		};
		if (st.kind == BN_STEP_ADD || st.kind == BN_STEP_MUL) {
			use(st.a);
			use((uint32_t)st.b);
		} else if (st.kind == BN_STEP_POW) {
			use(st.a);
		}
	}
	// slots: a result takes the lowest free slot at its step -- its operands still hold theirs -- and gives it back after its last use
	ct_program q;
	q.out_level = out_level;
	q.input_levels.assign(input_levels, input_levels + n_inputs);
	std::vector<uint32_t> operand(n, 0);
	std::vector<uint32_t> free_slots; // (kept sorted descending: back() is the lowest)
	uint32_t n_slots = 0;
	auto release = [&](uint32_t o, uint32_t s) {
		if ((operand[o] & kCtTagMask) != kCtSlot || last_use[o] != s) return;
		const uint32_t slot = operand[o] & kCtIdxMask;
		for (uint32_t f : free_slots)
			if (f == slot) return; // (an operand used twice by one step)
		size_t at = free_slots.size();
		free_slots.push_back(slot);
		while (at > 0 && free_slots[at - 1] < free_slots[at]) {
			const uint32_t t = free_slots[at - 1];
			free_slots[at - 1] = free_slots[at];
			free_slots[at] = t;
			at--;
		}
	};
	for (uint32_t s = 0; s < n; s++) {
		if (!live[s]) continue;
		const bn_step &st = steps[s];
		if (st.kind == BN_STEP_VAR) {
			operand[s] = kCtInput | st.a;
			continue;
		}
		if (st.kind == BN_STEP_CONST) {
			operand[s] = kCtConst | (uint32_t)q.consts.size();
			q.consts.push_back(ct_broadcast(f128{st.cst.lo, st.cst.hi}, out_level));
			continue;
		}
		uint32_t slot;
		if (!free_slots.empty()) {
			slot = free_slots.back();
			free_slots.pop_back();
		} else {
			slot = n_slots++;
			if (n_slots > BN_TOWER_EXPR_MAX_LIVE) return "more than BN_TOWER_EXPR_MAX_LIVE intermediate values are live at once";
		}
		operand[s] = kCtSlot | slot;
		ct_op op{};
		op.kind = st.kind;
		op.dst = slot;
		if (st.kind == BN_STEP_POW) {
			op.a = operand[st.a];
			op.b = op.a;
			op.exp = st.b;
			op.level = level[st.a];
			release(st.a, s);
		} else {
			const uint32_t sa = st.a, sb = (uint32_t)st.b;
			const bool a_narrow = st.kind == BN_STEP_MUL && level[sa] < level[sb];
			op.a = operand[a_narrow ? sb : sa];
			op.b = operand[a_narrow ? sa : sb];
			op.level = level[a_narrow ? sa : sb];
			release(sa, s);
			release(sb, s);
		}
		q.ops.push_back(op);
	}
	q.n_slots = n_slots;
	q.result = operand[n - 1];
	p = std::move(q);
	return nullptr;
}

// ---------------------------------------------------------------- arithmetic on an element of 2^(7 - L) values (host and device)

// the bit at position 0 of every 2^L-bit place of a 64-bit word (L <= 6)
BN_HD inline uint64_t ct_place_ones(uint32_t L)
{
	switch (L) {
	case 0: return ~0ull;
	case 1: return 0x5555555555555555ull;
	case 2: return 0x1111111111111111ull;
	case 3: return 0x0101010101010101ull;
	case 4: return 0x0001000100010001ull;
	case 5: return 0x0000000100000001ull;
	default: return 1ull;
	}
}

// ONE at every place
BN_HD inline f128 ct_one(uint32_t L)
{
	if (L == 7) return f128{1, 0};
	const uint64_t o = ct_place_ones(L);
	return f128{o, o};
}

// every place filled with bit S of its value, S < 8 a constant; at L = 7 the value is the whole element and only b.lo is looked at
// (the caller has shifted the bits it walks down to there)
template <int S>
BN_HD inline f128 ct_bit_mask(f128 b, uint32_t L)
{
	if (L == 7) {
		const uint64_t m = 0 - ((b.lo >> S) & 1);
		return f128{m, m};
	}
	const uint64_t ones = ct_place_ones(L);
	const uint32_t W = 1u << L; // <= 64
	const uint64_t x = (b.lo >> S) & ones, y = (b.hi >> S) & ones;
	return f128{((x << (W - 1)) << 1) - x, ((y << (W - 1)) << 1) - y}; // (2^W - 1) times the bit of every place
}

// mul_walk<K> of gf128.hpp on every place at once, K <= 3: the bits S .. S + 2^K - 1 of the places of b
template <int K, int S>
BN_HD inline f128 ct_walk(f128 a, f128 b, uint32_t L)
{
	if constexpr (K == 0) {
		const f128 m = ct_bit_mask<S>(b, L);
		return f128{a.lo & m.lo, a.hi & m.hi};
	} else {
		return ct_walk<K - 1, S>(a, b, L) ^ ct_walk<K - 1, S + (1 << (K - 1))>(mulx<K - 1>(a), b, L);
	}
}

// a * b in every place; the values of b lie in T_m, m <= L.  Above m = 3 the walk goes over the bytes of b's values: byte j of the
// walk multiplies a * 2^(8 j) (mul_basis: at most four multiplications by an X_k, 3 <= k < m <= L, which stay inside a place).
BN_HD inline f128 ct_mul(f128 a, f128 b, uint32_t m, uint32_t L)
{
	if (L == 0) return f128{a.lo & b.lo, a.hi & b.hi};
	switch (m) {
	case 0: return ct_walk<0, 0>(a, b, L);
	case 1: return ct_walk<1, 0>(a, b, L);
	case 2: return ct_walk<2, 0>(a, b, L);
	default: break;
	}
	f128 r = f128_zero();
	const uint32_t n_bytes = 1u << (m - 3); // <= 16
	for (uint32_t j = 0; j < n_bytes; j++) {
		const uint32_t sh = 8 * j;
		f128 bs;
		if (L == 7)
			bs = f128{sh >= 64 ? b.hi >> (sh - 64) : b.lo >> sh, 0};
		else
			bs = f128{b.lo >> sh, b.hi >> sh}; // (sh < 2^m <= 2^L <= 64)
		r ^= ct_walk<3, 0>(mul_basis(a, sh), bs, L);
	}
	return r;
}

// a^e in every place, a of level m: square and multiply over the 64 bits of e, highest first; the squarings of the leading ONE are
// skipped (e is the same in every lane)
BN_HD inline f128 ct_pow(f128 a, uint64_t e, uint32_t m, uint32_t L)
{
	if (L == 0) return e == 0 ? f128{~0ull, ~0ull} : a;
	f128 r = ct_one(L);
	bool started = false;
	for (int i = 63; i >= 0; i--) {
		if (started) r = ct_mul(r, r, m, L);
		if ((e >> i) & 1) {
			r = started ? ct_mul(r, a, m, L) : a;
			started = true;
		}
	}
	return r;
}

// The values of output element `at` that an input of level l = L - d holds: piece `at mod 2^d` of 2^(7 - d) bits of input element
// `at div 2^d` (x), every value moved to its place.  d = 0: the element itself.
BN_HD inline f128 ct_spread(f128 x, uint64_t at, uint32_t l, uint32_t L)
{
	const uint32_t d = L - l;
	if (d == 0) return x;
	const uint32_t piece_bits = 128u >> d; // <= 64
	const uint32_t off = (uint32_t)(at & ((1u << d) - 1)) * piece_bits;
	uint64_t piece = ((off & 64) ? x.hi : x.lo) >> (off & 63);
	if (piece_bits < 64) piece &= ((uint64_t)1 << piece_bits) - 1;
	if (L == 7) return f128{piece, 0};
	const uint32_t n = 128u >> L, w = 1u << l, W = 1u << L; // values, their bits, the bits of a place; w < W <= 64
	const uint64_t vm = ((uint64_t)1 << w) - 1;
	uint64_t lo = 0, hi = 0;
	for (uint32_t i = 0; i < n / 2; i++) {
		lo |= ((piece >> (i * w)) & vm) << (i * W);
		hi |= ((piece >> ((i + n / 2) * w)) & vm) << (i * W);
	}
	return f128{lo, hi};
}

} // namespace bn
