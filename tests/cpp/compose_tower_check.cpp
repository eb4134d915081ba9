// tests/cpp/compose_tower_check.cpp -- the tower-expression compiler and the packed-subfield arithmetic of
// binius_amd/csrc/compose_tower.hpp on the CPU, without a GPU and without the library: every case compiles a step list, runs the
// program on packed columns exactly as kernels_compose_tower.hip does (ct_spread, ct_mul, ct_pow on whole elements, slots in an
// array) and compares every value with the same steps evaluated value by value in B128 (mul_slow / pow_slow of gf128.hpp), which
// must come out below 2^(2^out_level).  The invalid tables must be rejected, each for its own reason.  Stand-alone (its own main),
// so it is also what a host sanitizer build runs: g++ -fsanitize=address,undefined with the same sources.
// Prints one line per group and "compose_tower_check ok"; exit status 1 on the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../binius_amd/csrc/compose_tower.hpp"

using bn::f128;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
	g_rng ^= g_rng << 13;
	g_rng ^= g_rng >> 7;
	g_rng ^= g_rng << 17;
	return g_rng;
}

static bn_step S(uint32_t kind, uint32_t a = 0, uint64_t b = 0, uint64_t lo = 0, uint64_t hi = 0)
{
	bn_step s{};
	s.kind = kind;
	s.a = a;
	s.b = b;
	s.cst.lo = lo;
	s.cst.hi = hi;
	return s;
}
static bn_step VAR(uint32_t v) { return S(BN_STEP_VAR, v); }
static bn_step CST(uint64_t lo, uint64_t hi = 0) { return S(BN_STEP_CONST, 0, 0, lo, hi); }
static bn_step ADD(uint32_t a, uint32_t b) { return S(BN_STEP_ADD, a, b); }
static bn_step MUL(uint32_t a, uint32_t b) { return S(BN_STEP_MUL, a, b); }
static bn_step POW(uint32_t a, uint64_t e) { return S(BN_STEP_POW, a, e); }

static f128 level_mask(uint32_t l)
{
	if (l == 7) return f128{~0ull, ~0ull};
	if (l == 6) return f128{~0ull, 0};
	return f128{((uint64_t)1 << (1u << l)) - 1, 0};
}
static f128 random_value(uint32_t l, int mode)
{
	const f128 m = level_mask(l);
	switch (mode) {
	case 1: return f128{0, 0};
	case 2: return m;
	case 3: return l == 0 ? f128{1, 0} : f128{2, 0};
	default: return f128{rnd() & m.lo, rnd() & m.hi};
	}
}
// value i of a column packed at level l
static f128 get_value(const std::vector<f128> &col, uint64_t i, uint32_t l)
{
	if (l == 7) return col[i];
	const uint64_t bit = i << l;
	const f128 e = col[bit >> 7];
	const uint64_t w = (bit & 64) ? e.hi : e.lo;
	return f128{(w >> (bit & 63)) & level_mask(l).lo, 0};
}
static void set_value(std::vector<f128> &col, uint64_t i, uint32_t l, f128 v)
{
	if (l == 7) {
		col[i] = v;
		return;
	}
	const uint64_t bit = i << l;
	uint64_t &w = (bit & 64) ? col[bit >> 7].hi : col[bit >> 7].lo;
	w |= v.lo << (bit & 63);
}
static uint64_t col_elems(uint64_t n, uint32_t l) { return ((n << l) >> 7) ? (n << l) >> 7 : 1; }

static int g_cases = 0;

// compile + run on n values + compare; returns false (and says why) on a difference
static bool run_case(const char *name, const std::vector<bn_step> &steps, const std::vector<uint32_t> &in_levels, uint32_t L, uint64_t n, int mode = 0)
{
	bn::ct_program p;
	const char *why = bn::ct_compile(steps.data(), steps.size(), in_levels.data(), (uint32_t)in_levels.size(), L, p);
	if (why) {
		std::printf("FAIL %s: rejected: %s\n", name, why);
		return false;
	}
	std::vector<std::vector<f128>> cols(in_levels.size());
	for (size_t v = 0; v < cols.size(); v++) {
		cols[v].assign(col_elems(n, in_levels[v]), f128{0, 0});
		for (uint64_t i = 0; i < n; i++) set_value(cols[v], i, in_levels[v], random_value(in_levels[v], mode == 3 && v != 0 ? 0 : mode));
	}
	const uint64_t out_elems = col_elems(n, L);
	if ((n << L) < 128) {
		std::printf("FAIL %s: output below one element\n", name);
		return false;
	}
	std::vector<f128> out(out_elems);
	for (uint64_t at = 0; at < out_elems; at++) {
		f128 slot[BN_TOWER_EXPR_MAX_LIVE];
		auto fetch = [&](uint32_t o) {
			const uint32_t idx = o & bn::kCtIdxMask;
			if ((o & bn::kCtTagMask) == bn::kCtSlot) return slot[idx];
			if ((o & bn::kCtTagMask) == bn::kCtConst) return p.consts[idx];
			const uint32_t l = p.input_levels[idx];
			return bn::ct_spread(cols[idx][at >> (L - l)], at, l, L);
		};
		for (const bn::ct_op &op : p.ops) {
			f128 a = fetch(op.a);
			if (op.kind == BN_STEP_ADD)
				a ^= fetch(op.b);
			else if (op.kind == BN_STEP_MUL)
				a = bn::ct_mul(a, fetch(op.b), op.level, L);
			else
				a = bn::ct_pow(a, op.exp, op.level, L);
			if (op.dst >= p.n_slots) {
				std::printf("FAIL %s: slot %u of %u\n", name, op.dst, p.n_slots);
				return false;
			}
			slot[op.dst] = a;
		}
		out[at] = fetch(p.result);
	}
	// value by value in B128
	std::vector<f128> val(steps.size());
	const f128 m = level_mask(L);
	for (uint64_t i = 0; i < n; i++) {
		for (size_t s = 0; s < steps.size(); s++) {
			const bn_step &st = steps[s];
			switch (st.kind) {
			case BN_STEP_VAR: val[s] = get_value(cols[st.a], i, in_levels[st.a]); break;
			case BN_STEP_CONST: val[s] = f128{st.cst.lo, st.cst.hi}; break;
			case BN_STEP_ADD: val[s] = val[st.a] ^ val[st.b]; break;
			case BN_STEP_MUL: val[s] = bn::mul_slow(val[st.a], val[st.b]); break;
			default: val[s] = bn::pow_slow(val[st.a], st.b); break;
			}
		}
		const f128 want = val.back();
		if ((want.lo & ~m.lo) || (want.hi & ~m.hi)) {
			std::printf("FAIL %s: value %llu leaves T_%u\n", name, (unsigned long long)i, L);
			return false;
		}
		const f128 got = get_value(out, i, L);
		if (!(got == want)) {
			std::printf("FAIL %s: value %llu: got %016llx%016llx want %016llx%016llx\n", name, (unsigned long long)i, (unsigned long long)got.hi,
			            (unsigned long long)got.lo, (unsigned long long)want.hi, (unsigned long long)want.lo);
			return false;
		}
	}
	g_cases++;
	return true;
}

static bool expect_reject(const char *name, const bn_step *steps, uint64_t n_steps, const uint32_t *levels, uint32_t n_inputs, uint32_t L, const char *needle)
{
	bn::ct_program p;
	p.n_slots = 77; // (a rejected expression leaves the program alone)
	const char *why = bn::ct_compile(steps, n_steps, levels, n_inputs, L, p);
	if (!why || !std::strstr(why, needle) || p.n_slots != 77) {
		std::printf("FAIL invalid table %s: %s\n", name, why ? why : "accepted");
		return false;
	}
	g_cases++;
	return true;
}

// sum of bit_i * 2^i over n_bits B1 inputs, left-deep (pack_fp / pack_b8: VAR, CONST, MUL, ADD per term)
static std::vector<bn_step> pack_steps(uint32_t n_bits)
{
	std::vector<bn_step> st;
	uint32_t acc = 0;
	for (uint32_t i = 0; i < n_bits; i++) {
		st.push_back(VAR(i));
		st.push_back(i < 64 ? CST((uint64_t)1 << i) : CST(0, (uint64_t)1 << (i - 64)));
		st.push_back(MUL((uint32_t)st.size() - 2, (uint32_t)st.size() - 1));
		if (i) st.push_back(ADD(acc, (uint32_t)st.size() - 1));
		acc = (uint32_t)st.size() - 1;
	}
	return st;
}

int main()
{
	static const uint32_t kLevels[] = {0, 3, 4, 5, 6, 7};
	bool ok = true;
	// ---- x * c + d for every pair of levels, every data mode; sizes: one output element, and several
	for (uint32_t L : kLevels)
		for (uint32_t l : kLevels) {
			if (l > L) continue;
			for (int mode = 0; mode < 3; mode++)
				for (uint64_t n : {(uint64_t)128 >> L, (uint64_t)(128 >> L) * 8}) {
					const f128 c = random_value(L, 0), d = random_value(L, 0);
					std::vector<bn_step> st{VAR(0), CST(c.lo, c.hi), MUL(0, 1), CST(d.lo, d.hi), ADD(2, 3)};
					ok = ok && run_case(("affine " + std::to_string(l) + "->" + std::to_string(L)).c_str(), st, {l}, L, n, mode);
				}
		}
	std::printf("affine: %d cases\n", g_cases);
	// ---- products of two inputs, either order, with the generator as one operand
	for (uint32_t L : kLevels)
		for (uint32_t l : kLevels) {
			if (l > L) continue;
			for (int mode = 0; mode < 4; mode++) {
				ok = ok && run_case("mul narrow left", {VAR(0), VAR(1), MUL(0, 1)}, {l, L}, L, (uint64_t)(128 >> L) * 4, mode);
				ok = ok && run_case("mul narrow right", {VAR(0), VAR(1), MUL(0, 1)}, {L, l}, L, (uint64_t)(128 >> L) * 4, mode);
			}
		}
	// ---- powers
	for (uint32_t L : {3u, 6u})
		for (uint64_t e : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)254, ~(uint64_t)0})
			for (int mode = 0; mode < 3; mode++) ok = ok && run_case("pow", {VAR(0), POW(0, e)}, {L}, L, (uint64_t)(128 >> L) * 2, mode);
	for (uint64_t e : {(uint64_t)0, (uint64_t)5}) ok = ok && run_case("pow B1", {VAR(0), POW(0, e)}, {0}, 0, 256);
	ok = ok && run_case("pow below the output level", {VAR(0), POW(0, 7), VAR(1), MUL(1, 2)}, {3, 5}, 5, 64);
	// ---- constants of level 1 and 2, roots that hold no slot, a repeated variable, an unused input, dead steps
	ok = ok && run_case("const levels", {VAR(0), CST(2), MUL(0, 1), CST(9), MUL(2, 3), CST(1), ADD(4, 5)}, {3}, 3, 64);
	ok = ok && run_case("root var (upcast)", {VAR(0)}, {3}, 5, 64);
	ok = ok && run_case("root const", {VAR(0), CST(0xabcd)}, {3}, 4, 64);
	ok = ok && run_case("repeated variable", {VAR(0), MUL(0, 0), ADD(1, 1), ADD(2, 0), MUL(3, 3)}, {4}, 4, 32);
	ok = ok && run_case("unused input", {VAR(1), CST(3), MUL(0, 1)}, {5, 3, 0}, 3, 64);
	ok = ok && run_case("dead steps", {VAR(0), VAR(1), MUL(0, 1), POW(2, 77), ADD(0, 1)}, {3, 3}, 3, 64);
	// ---- gadget shapes
	{
		std::vector<uint32_t> bits32(32, 0), bits64(64, 0), bits8(8, 0), bits128(128, 0);
		ok = ok && run_case("pack_fp B32", pack_steps(32), bits32, 5, 256);
		ok = ok && run_case("pack_fp B64", pack_steps(64), bits64, 6, 256);
		ok = ok && run_case("pack_b8", pack_steps(8), bits8, 3, 256);
		const std::vector<bn_step> p128 = pack_steps(128);
		ok = ok && p128.size() == 511 && run_case("pack B128 (511 steps)", p128, bits128, 7, 128);
		ok = ok && run_case("a + s (a + b) at B1", {VAR(0), VAR(1), VAR(2), ADD(0, 1), MUL(2, 3), ADD(0, 4)}, {0, 0, 0}, 0, 1024);
		ok = ok && run_case("x + ONE at B32", {VAR(0), CST(1), ADD(0, 1)}, {5}, 5, 256);
		ok = ok && run_case("five-term sum at B1", {VAR(0), VAR(1), VAR(2), VAR(3), VAR(4), ADD(0, 1), ADD(5, 2), ADD(6, 3), ADD(7, 4)}, {0, 0, 0, 0, 0}, 0, 1024);
	}
	// ---- slots: a balanced sum of 32 products; 17 products alive at once
	{
		std::vector<bn_step> st;
		std::vector<uint32_t> lv(64, 4);
		for (uint32_t i = 0; i < 64; i++) st.push_back(VAR(i));
		// post-order over the balanced tree keeps few values alive
		struct rec {
			static uint32_t build(std::vector<bn_step> &st, uint32_t lo, uint32_t hi)
			{
				if (hi - lo == 1) {
					st.push_back(MUL(2 * lo, 2 * lo + 1));
					return (uint32_t)st.size() - 1;
				}
				const uint32_t a = build(st, lo, (lo + hi) / 2), b = build(st, (lo + hi) / 2, hi);
				st.push_back(ADD(a, b));
				return (uint32_t)st.size() - 1;
			}
		};
		rec::build(st, 0, 32);
		ok = ok && run_case("balanced sum of 32 products", st, lv, 4, 64);
		std::vector<bn_step> wide;
		for (uint32_t i = 0; i < 34; i++) wide.push_back(VAR(i));
		for (uint32_t i = 0; i < 17; i++) wide.push_back(MUL(2 * i, 2 * i + 1));
		for (uint32_t i = 1; i < 17; i++) wide.push_back(ADD(i == 1 ? 34 : (uint32_t)wide.size() - 1, 34 + i));
		ok = ok && expect_reject("17 live slots", wide.data(), wide.size(), lv.data(), 64, 4, "live");
		// (one product fewer fits)
		std::vector<bn_step> fits;
		for (uint32_t i = 0; i < 32; i++) fits.push_back(VAR(i));
		for (uint32_t i = 0; i < 15; i++) fits.push_back(MUL(2 * i, 2 * i + 1));
		for (uint32_t i = 1; i < 15; i++) fits.push_back(ADD(i == 1 ? 32 : (uint32_t)fits.size() - 1, 32 + i));
		ok = ok && run_case("15 products then their sum", fits, lv, 4, 64);
	}
	// ---- seeded random DAGs over mixed levels
	for (uint32_t seed = 0; seed < 200 && ok; seed++) {
		g_rng = 0xD1B54A32D192ED03ull * (seed + 1);
		const uint32_t L = kLevels[rnd() % 6];
		const uint32_t n_in = 1 + rnd() % 4;
		std::vector<uint32_t> lv(n_in);
		for (uint32_t &x : lv) {
			do x = kLevels[rnd() % 6];
			while (x > L);
		}
		std::vector<bn_step> st;
		const uint32_t n_steps = 1 + rnd() % 24;
		for (uint32_t s = 0; s < n_steps; s++) {
			const uint32_t k = s < 2 ? (uint32_t)(rnd() % 2) : (uint32_t)(rnd() % 7);
			if (k == 0)
				st.push_back(VAR((uint32_t)(rnd() % n_in)));
			else if (k == 1) {
				const f128 c = random_value((uint32_t)(rnd() % (L + 1)), 0);
				st.push_back(CST(c.lo, c.hi));
			} else if (k <= 3)
				st.push_back(ADD((uint32_t)(rnd() % s), (uint32_t)(rnd() % s)));
			else if (k <= 5)
				st.push_back(MUL((uint32_t)(rnd() % s), (uint32_t)(rnd() % s)));
			else
				st.push_back(POW((uint32_t)(rnd() % s), rnd() % 5 == 0 ? rnd() : rnd() % 9));
		}
		ok = ok && run_case(("random DAG " + std::to_string(seed)).c_str(), st, lv, L, (uint64_t)(128 >> L) * 4);
	}
	std::printf("valid: %d cases\n", g_cases);
	// ---- the invalid tables
	{
		const uint32_t lv[2] = {3, 0};
		const bn_step one[] = {VAR(0)};
		ok = ok && expect_reject("null steps", nullptr, 1, lv, 1, 3, "null");
		ok = ok && expect_reject("null levels", one, 1, nullptr, 1, 3, "null");
		ok = ok && expect_reject("no steps", one, 0, lv, 1, 3, "number of steps");
		std::vector<bn_step> many(BN_TOWER_EXPR_MAX_STEPS + 1, VAR(0));
		ok = ok && expect_reject("too many steps", many.data(), many.size(), lv, 1, 3, "number of steps");
		std::vector<uint32_t> lots(BN_TOWER_EXPR_MAX_INPUTS + 1, 0);
		ok = ok && expect_reject("too many inputs", one, 1, lots.data(), (uint32_t)lots.size(), 3, "inputs");
		const bn_step fwd[] = {VAR(0), ADD(0, 1)};
		ok = ok && expect_reject("operand not earlier", fwd, 2, lv, 1, 3, "later step");
		const bn_step fwd2[] = {VAR(0), POW(1, 2)};
		ok = ok && expect_reject("pow base not earlier", fwd2, 2, lv, 1, 3, "later step");
		const bn_step far[] = {VAR(0), S(BN_STEP_MUL, 0, (uint64_t)1 << 32)};
		ok = ok && expect_reject("operand beyond 32 bits", far, 2, lv, 1, 3, "later step");
		const bn_step var2[] = {VAR(2)};
		ok = ok && expect_reject("variable index", var2, 1, lv, 2, 3, "variable index");
		const bn_step unk[] = {VAR(0), S(9, 0, 0)};
		ok = ok && expect_reject("unknown kind", unk, 2, lv, 1, 3, "unknown");
		for (uint32_t bad : {1u, 2u, 8u}) {
			const uint32_t lb[1] = {bad};
			ok = ok && expect_reject("input level", one, 1, lb, 1, 7, "input's tower level");
			ok = ok && expect_reject("output level", one, 1, lv, 1, bad, "output's tower level");
		}
		ok = ok && expect_reject("input above the output", one, 1, lv, 1, 0, "above the output");
		const bn_step big[] = {VAR(1), CST(256), ADD(0, 1)};
		ok = ok && expect_reject("constant above the output", big, 3, lv, 2, 3, "above the output");
	}
	if (!ok) return 1;
	std::printf("compose_tower_check ok: %d cases\n", g_cases);
	return 0;
}
