// tests/cpp/compose_batch_check.cpp -- the plan of a batch of tower-typed expressions (binius_amd/csrc/compose_batch.hpp) on the CPU,
// without a GPU and without the library.  Every case compiles its members, plans the batch, fills the upload's sections and then walks
// EVERY unit of the grid the way k_compose_tower_batch does: the job by bisection over `start`, the job's elements-per-thread class,
// the chunk loop over 256 threads with the slots in an array indexed like the kernel's LDS (and bounded by the launch's LDS size), the
// clamped loads and the predicated store into an arena with guard elements between the outputs.  Each job's output must equal the same
// program run alone, element by element (compose_tower.hpp's ct_spread / ct_mul / ct_pow; those are checked against B128 arithmetic by
// compose_tower_check.cpp), and every guard must be untouched.  The invalid batches and calls must be rejected, each for its own reason.
// Stand-alone (its own main), so it is also what a host sanitizer build runs: g++ -fsanitize=address,undefined with the same sources.
// Prints "compose_batch_check ok: N cases"; exit status 1 on the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../binius_amd/csrc/compose_batch.hpp"

using bn::f128;

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint64_t rnd()
{
	g_rng ^= g_rng << 13;
	g_rng ^= g_rng >> 7;
	g_rng ^= g_rng << 17;
	return g_rng;
}

static bn_step S(uint32_t kind, uint32_t a = 0, uint64_t b = 0, uint64_t lo = 0)
{
	bn_step s{};
	s.kind = kind;
	s.a = a;
	s.b = b;
	s.cst.lo = lo;
	return s;
}
static bn_step VAR(uint32_t v) { return S(BN_STEP_VAR, v); }
static bn_step CST(uint64_t lo) { return S(BN_STEP_CONST, 0, 0, lo); }
static bn_step ADD(uint32_t a, uint32_t b) { return S(BN_STEP_ADD, a, b); }
static bn_step MUL(uint32_t a, uint32_t b) { return S(BN_STEP_MUL, a, b); }
static bn_step POW(uint32_t a, uint64_t e) { return S(BN_STEP_POW, a, e); }

static const f128 kGuard{0xA5A5A5A5DEADBEEFull, 0x0123456789ABCDEFull};
static int g_cases = 0;

#define CHECK(cond, ...)                    \
	do {                                    \
		if (!(cond)) {                      \
			std::printf("FAIL %s: ", name); \
			std::printf(__VA_ARGS__);       \
			std::printf("\n");              \
			return false;                   \
		}                                   \
	} while (0)

struct Member {
	std::vector<bn_step> steps;
	std::vector<uint32_t> levels;
	uint32_t out_level;
};
static const Member kSelect{{VAR(0), VAR(1), VAR(2), ADD(0, 1), MUL(2, 3), ADD(0, 4)}, {0, 0, 0}, 0}; // a + s (a + b), the mul gadget's

// k independent products of input pairs, all computed before the first sum: k + 1 slots are live at the first sum
static Member products(uint32_t k, const std::vector<uint32_t> &pair_levels, uint32_t out_level)
{
	Member m;
	m.out_level = out_level;
	for (uint32_t i = 0; i < 2 * k; i++) {
		m.steps.push_back(VAR(i));
		m.levels.push_back(pair_levels[i % pair_levels.size()]);
	}
	for (uint32_t i = 0; i < k; i++) m.steps.push_back(MUL(2 * i, 2 * i + 1));
	uint32_t acc = 2 * k;
	m.steps.push_back(ADD(acc, k == 1 ? 0 : acc + 1));
	acc = (uint32_t)m.steps.size() - 1;
	for (uint32_t i = 2; i < k; i++) {
		m.steps.push_back(ADD(acc, 2 * k + i));
		acc = (uint32_t)m.steps.size() - 1;
	}
	return m;
}

static uint64_t col_elems(uint32_t n_vars, uint32_t l) { return bn::cb_column_elems(n_vars, l); }

// the program alone, element by element
static std::vector<f128> run_alone(const bn::ct_program &p, const uint64_t *rows, uint64_t out_elems)
{
	const uint32_t L = p.out_level;
	std::vector<f128> out(out_elems);
	for (uint64_t at = 0; at < out_elems; at++) {
		f128 slot[BN_TOWER_EXPR_MAX_LIVE];
		auto fetch = [&](uint32_t o) {
			const uint32_t idx = o & bn::kCtIdxMask;
			if ((o & bn::kCtTagMask) == bn::kCtSlot) return slot[idx];
			if ((o & bn::kCtTagMask) == bn::kCtConst) return p.consts[idx];
			const uint32_t l = p.input_levels[idx];
			return bn::ct_spread(((const f128 *)(uintptr_t)rows[idx])[at >> (L - l)], at, l, L);
		};
		for (const bn::ct_op &op : p.ops) {
			f128 a = fetch(op.a);
			if (op.kind == BN_STEP_ADD)
				a ^= fetch(op.b);
			else if (op.kind == BN_STEP_MUL)
				a = bn::ct_mul(a, fetch(op.b), op.level, L);
			else
				a = bn::ct_pow(a, op.exp, op.level, L);
			slot[op.dst] = a;
		}
		out[at] = fetch(p.result);
	}
	return out;
}

// batch.hpp's find_job
static uint32_t find_job(const bn::compose_batch_job *jobs, uint32_t n_jobs, uint32_t u)
{
	uint32_t lo = 0, hi = n_jobs;
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (jobs[mid].start <= u)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// the grid of k_compose_tower_batch over the uploaded sections; false if an index leaves the LDS, a section or a job's output
static bool walk_grid(const char *name, const bn::compose_batch_plan &p, const uint64_t *rows, f128 *arena)
{
	std::vector<bn::ct_op> ops(p.n_ops);
	std::vector<f128> consts(p.n_consts);
	std::vector<uint32_t> levels(p.n_levels);
	bn::cb_fill(p, ops.data(), consts.data(), levels.data());
	const std::vector<bn::compose_batch_job> &jobs = p.jobs;
	CHECK(p.lds_bytes <= (64u << 10) && p.lds_bytes % 4 == 0, "LDS of %u bytes", p.lds_bytes);
	CHECK(jobs[0].start == 0, "the first job does not start at unit 0");
	std::vector<uint32_t> lds(p.lds_bytes / 4);
	for (uint32_t unit = 0; unit < p.total_units; unit++) {
		const bn::compose_batch_job &job = jobs[find_job(jobs.data(), (uint32_t)jobs.size(), unit)];
		const uint32_t Q = job.q, L = job.out_level;
		CHECK(Q == 4 || Q == 2 || Q == 1, "class %u", Q);
		CHECK(job.start <= unit && (uint64_t)(unit - job.start) * bn::kComposeUnitElems < job.out_elems, "unit %u is outside its job", unit);
		CHECK((uint64_t)job.ops_off + job.n_ops <= ops.size(), "ops leave their section");
		const bn::ct_op *jops = ops.data() + job.ops_off;
		const uint64_t len = job.out_elems, unit_first = (uint64_t)(unit - job.start) * bn::kComposeUnitElems;
		const uint32_t chunk = 256 * Q;
		for (uint32_t c = 0; c < bn::kComposeUnitElems / chunk; c++) {
			const uint64_t first = unit_first + (uint64_t)c * chunk;
			if (first >= len) break;
			for (uint32_t tid = 0; tid < 256; tid++)
				for (uint32_t q = 0; q < Q; q++) {
					const uint64_t j = first + tid + 256 * q, at = j < len ? j : len - 1;
					bool ok = true;
					auto word = [&](uint32_t slot, uint32_t w) -> uint32_t & {
						const size_t i = (size_t)((slot * Q + q) * 4 + w) * 256 + tid;
						if (i >= lds.size()) {
							ok = false;
							return lds[0];
						}
						return lds[i];
					};
					auto fetch = [&](uint32_t o) {
						const uint32_t idx = o & bn::kCtIdxMask;
						if ((o & bn::kCtTagMask) == bn::kCtSlot)
							return f128{(uint64_t)word(idx, 0) | ((uint64_t)word(idx, 1) << 32), (uint64_t)word(idx, 2) | ((uint64_t)word(idx, 3) << 32)};
						if ((o & bn::kCtTagMask) == bn::kCtConst) {
							if ((size_t)job.consts_off + idx >= consts.size()) {
								ok = false;
								return f128{0, 0};
							}
							return consts[job.consts_off + idx];
						}
						if ((size_t)job.levels_off + idx >= levels.size()) {
							ok = false;
							return f128{0, 0};
						}
						const uint32_t l = levels[job.levels_off + idx];
						return bn::ct_spread(((const f128 *)(uintptr_t)rows[job.first_row + idx])[at >> (L - l)], at, l, L);
					};
					for (uint32_t i = 0; i < job.n_ops; i++) {
						const bn::ct_op &op = jops[i];
						f128 a = fetch(op.a);
						if (op.kind == BN_STEP_ADD)
							a ^= fetch(op.b);
						else if (op.kind == BN_STEP_MUL)
							a = bn::ct_mul(a, fetch(op.b), op.level, L);
						else
							a = bn::ct_pow(a, op.exp, op.level, L);
						word(op.dst, 0) = (uint32_t)a.lo;
						word(op.dst, 1) = (uint32_t)(a.lo >> 32);
						word(op.dst, 2) = (uint32_t)a.hi;
						word(op.dst, 3) = (uint32_t)(a.hi >> 32);
					}
					const f128 r = fetch(job.result);
					CHECK(ok, "unit %u: an index leaves the LDS or a section", unit);
					if (j < len) arena[job.out_offset + j] = r;
				}
		}
	}
	return true;
}

struct JobSpec {
	uint32_t member;
	uint32_t n_vars;
	int share_rows_with; // -1: rows of its own; j: the rows of job j (the same first_row)
};

// compile, plan, lay the outputs out with one guard element around each, walk, compare with every program alone
static bool run_batch(const char *name, const std::vector<Member> &members, const std::vector<JobSpec> &specs, uint32_t want_programs, const std::vector<uint32_t> &want_slots = {})
{
	g_cases++;
	std::vector<bn::ct_program> progs(members.size());
	std::vector<const bn::ct_program *> pp;
	for (size_t m = 0; m < members.size(); m++) {
		const uint32_t none = 0;
		const char *why = bn::ct_compile(members[m].steps.data(), members[m].steps.size(), members[m].levels.empty() ? &none : members[m].levels.data(),
		                                 (uint32_t)members[m].levels.size(), members[m].out_level, progs[m]);
		CHECK(!why, "member %zu rejected: %s", m, why);
		if (!want_slots.empty()) CHECK(progs[m].n_slots == want_slots[m], "member %zu has %u live slots, not %u", m, progs[m].n_slots, want_slots[m]);
		pp.push_back(&progs[m]);
	}
	std::vector<std::vector<f128>> cols; // every row's data
	std::vector<uint64_t> rows;
	std::vector<bn_compose_job> jobs;
	uint64_t arena_len = 1;
	for (size_t j = 0; j < specs.size(); j++) {
		const Member &m = members[specs[j].member];
		bn_compose_job jb{};
		jb.expr = specs[j].member;
		jb.n_vars = specs[j].n_vars;
		jb.out_offset = arena_len;
		arena_len += col_elems(jb.n_vars, m.out_level) + 1;
		if (specs[j].share_rows_with >= 0) {
			jb.first_row = jobs[specs[j].share_rows_with].first_row;
		} else {
			jb.first_row = (uint32_t)rows.size();
			for (size_t v = 0; v < m.levels.size(); v++) {
				const uint64_t n = col_elems(jb.n_vars, m.levels[v]);
				std::vector<f128> col(n);
				for (f128 &x : col) x = f128{rnd(), rnd()};
				if (n == 1 && jb.n_vars + m.levels[v] < 7) { // below one element: the low bits of one element, zeros above
					const uint32_t bits = 1u << (jb.n_vars + m.levels[v]);
					col[0].hi = 0;
					col[0].lo &= (((uint64_t)1 << (bits - 1)) << 1) - 1;
				}
				cols.push_back(std::move(col));
				rows.push_back(0);
			}
		}
		jobs.push_back(jb);
	}
	for (size_t r = 0, c = 0; r < rows.size(); r++, c++) rows[r] = (uint64_t)(uintptr_t)cols[c].data();
	bn::compose_batch_plan plan;
	const char *why = bn::cb_plan(pp.data(), (uint32_t)pp.size(), jobs.data(), (uint32_t)jobs.size(), plan);
	CHECK(!why, "batch rejected: %s", why);
	CHECK(plan.programs.size() == want_programs, "%zu distinct programs, not %u", plan.programs.size(), want_programs);
	CHECK(plan.n_rows == rows.size(), "the batch wants %u rows of %zu", plan.n_rows, rows.size());
	uint32_t lds = 0;
	uint64_t units = 0;
	for (size_t j = 0; j < jobs.size(); j++) {
		const bn::ct_program &p = progs[jobs[j].expr];
		lds = std::max(lds, bn::compose_tower_lds_bytes(p.n_slots));
		CHECK(plan.jobs[j].q == bn::compose_tower_per_thread(p.n_slots) && plan.jobs[j].start == units, "job %zu: class or first unit", j);
		units += (plan.jobs[j].out_elems + bn::kComposeUnitElems - 1) / bn::kComposeUnitElems;
	}
	CHECK(plan.lds_bytes == lds && plan.total_units == units, "LDS %u (want %u), units %u (want %llu)", plan.lds_bytes, lds, plan.total_units, (unsigned long long)units);
	std::vector<f128> arena(arena_len, kGuard);
	why = bn::cb_check_call(plan, rows.empty() ? &arena_len : rows.data(), (uint32_t)rows.size(), arena_len, (uint64_t)(uintptr_t)arena.data(), arena_len);
	CHECK(!why, "call rejected: %s", why);
	if (!walk_grid(name, plan, rows.data(), arena.data())) return false;
	std::vector<char> written(arena_len, 0);
	for (size_t j = 0; j < jobs.size(); j++) {
		const bn::ct_program &p = progs[jobs[j].expr];
		const uint64_t n = col_elems(jobs[j].n_vars, p.out_level);
		const std::vector<f128> want = run_alone(p, rows.data() + jobs[j].first_row, n);
		for (uint64_t i = 0; i < n; i++) {
			const f128 got = arena[jobs[j].out_offset + i];
			CHECK(got.lo == want[i].lo && got.hi == want[i].hi, "job %zu element %llu differs from the program alone", j, (unsigned long long)i);
			written[jobs[j].out_offset + i] = 1;
		}
	}
	for (uint64_t i = 0; i < arena_len; i++)
		if (!written[i]) CHECK(arena[i].lo == kGuard.lo && arena[i].hi == kGuard.hi, "guard element %llu was written", (unsigned long long)i);
	return true;
}

static bool expect(const char *name, const char *why, const char *want)
{
	g_cases++;
	CHECK(why != nullptr, "accepted, expected: %s", want);
	CHECK(std::strstr(why, want) != nullptr, "rejected with \"%s\", expected \"%s\"", why, want);
	return true;
}

static bool rejections()
{
	bn::ct_program sel, b32;
	const uint32_t lv5[2] = {5, 5};
	const bn_step mul[3] = {VAR(0), VAR(1), MUL(0, 1)};
	if (bn::ct_compile(kSelect.steps.data(), kSelect.steps.size(), kSelect.levels.data(), 3, 0, sel) || bn::ct_compile(mul, 3, lv5, 2, 5, b32)) return false;
	const bn::ct_program *pp[3] = {&sel, &b32, nullptr};
	bn::compose_batch_plan plan;
	auto J = [](uint32_t e, uint32_t first_row, uint32_t n_vars, uint64_t off, uint32_t reserved = 0) { return bn_compose_job{e, first_row, n_vars, reserved, off}; };
	bool ok = true;
	// ---- what the jobs alone decide (bn_expr_compile_tower_batch)
	bn_compose_job one[1] = {J(0, 0, 10, 0)};
	ok &= expect("null programs", bn::cb_plan(nullptr, 3, one, 1, plan), "null argument");
	ok &= expect("null jobs", bn::cb_plan(pp, 3, nullptr, 1, plan), "null argument");
	ok &= expect("no jobs", bn::cb_plan(pp, 3, one, 0, plan), "number of jobs");
	{
		std::vector<bn_compose_job> many(BN_COMPOSE_BATCH_MAX_JOBS + 1);
		for (size_t j = 0; j < many.size(); j++) many[j] = J(0, 0, 7, j);
		ok &= expect("jobs above the cap", bn::cb_plan(pp, 3, many.data(), (uint32_t)many.size(), plan), "number of jobs");
		g_cases++;
		if (bn::cb_plan(pp, 3, many.data(), BN_COMPOSE_BATCH_MAX_JOBS, plan) || plan.total_units != BN_COMPOSE_BATCH_MAX_JOBS || plan.programs.size() != 1) {
			std::printf("FAIL the cap itself is taken\n");
			ok = false;
		}
	}
	one[0] = J(3, 0, 10, 0);
	ok &= expect("expr index", bn::cb_plan(pp, 3, one, 1, plan), "not below n_exprs");
	one[0] = J(2, 0, 10, 0);
	ok &= expect("member of another kind", bn::cb_plan(pp, 3, one, 1, plan), "not a tower expression");
	one[0] = J(0, 0, 10, 0, 1);
	ok &= expect("reserved", bn::cb_plan(pp, 3, one, 1, plan), "reserved");
	one[0] = J(0, 0, BN_PE_MAX_VARS + 1, 0);
	ok &= expect("n_vars", bn::cb_plan(pp, 3, one, 1, plan), "BN_PE_MAX_VARS");
	one[0] = J(0, 0, 6, 0);
	ok &= expect("below one element", bn::cb_plan(pp, 3, one, 1, plan), "at least one 128-bit element");
	one[0] = J(1, 0, 1, 0); // 2 x 32 bits
	ok &= expect("below one element (B32)", bn::cb_plan(pp, 3, one, 1, plan), "at least one 128-bit element");
	bn_compose_job two[2] = {J(0, 0, 10, 0), J(1, 3, 3, 7)}; // 8 elements at 0, 2 at 7
	ok &= expect("outputs overlap", bn::cb_plan(pp, 3, two, 2, plan), "outputs overlap");
	two[1] = J(0, 0, 10, 0);
	ok &= expect("outputs equal", bn::cb_plan(pp, 3, two, 2, plan), "outputs overlap");
	two[0] = J(1, 0, 35, 0); // 2^33 elements: 2^23 units each -- fine; 2^40 values at B128 are 2^30 units each
	two[1] = J(1, 0, 35, (uint64_t)1 << 33);
	g_cases++;
	if (bn::cb_plan(pp, 3, two, 2, plan) || plan.total_units != (1u << 24)) {
		std::printf("FAIL two large jobs are taken\n");
		ok = false;
	}
	{
		std::vector<bn_compose_job> big(256);
		for (size_t j = 0; j < big.size(); j++) big[j] = J(1, 0, BN_PE_MAX_VARS, (uint64_t)j << 38); // 2^38 elements, 2^28 units each: 8 of them are 2^31
		ok &= expect("units", bn::cb_plan(pp, 3, big.data(), 8, plan), "31 bits");
		g_cases++;
		if (bn::cb_plan(pp, 3, big.data(), 7, plan) || plan.total_units != 7u << 28) {
			std::printf("FAIL seven such jobs are taken\n");
			ok = false;
		}
	}
	one[0] = J(0, 0xfffffffeu, 10, 0);
	ok &= expect("rows leave 32 bits", bn::cb_plan(pp, 3, one, 1, plan), "rows leave 32 bits");
	// a rejected plan leaves the caller's object alone
	// ---- what the pointers of a call decide (bn_compute_composite): two jobs, select at 2^10 bits (8 elements) and the B32 product at 2^3
	two[0] = J(0, 0, 10, 16);
	two[1] = J(1, 3, 3, 32);
	if (bn::cb_plan(pp, 3, two, 2, plan)) {
		std::printf("FAIL the plan of the call cases is rejected\n");
		return false;
	}
	const uint64_t out = 0x100000, len = 64; // the arena: [0x100000, 0x100400)
	const uint64_t good[5] = {0x200000, 0x200100, 0x200200, 0x200300, 0x200400};
	uint64_t r[5];
	auto reset = [&]() { std::memcpy(r, good, sizeof r); };
	g_cases++;
	if (const char *why = bn::cb_check_call(plan, good, 5, len, out, len)) {
		std::printf("FAIL the good call is rejected: %s\n", why);
		ok = false;
	}
	reset();
	r[1] = out + 16 * 8; // a row INSIDE the arena, below job 0's output: taken
	r[4] = out + 16 * 34;
	g_cases++;
	if (const char *why = bn::cb_check_call(plan, r, 5, len, out, len)) {
		std::printf("FAIL rows inside the arena are rejected: %s\n", why);
		ok = false;
	}
	ok &= expect("null rows", bn::cb_check_call(plan, nullptr, 5, len, out, len), "null argument");
	ok &= expect("null out", bn::cb_check_call(plan, good, 5, len, 0, len), "null argument");
	ok &= expect("row_len != out_len", bn::cb_check_call(plan, good, 5, len - 1, out, len), "row_len must equal out_len");
	ok &= expect("n_rows too small", bn::cb_check_call(plan, good, 4, len, out, len), "more rows");
	ok &= expect("misaligned out", bn::cb_check_call(plan, good, 5, len, out + 8, len), "misaligned pointer");
	ok &= expect("a range leaves the arena", bn::cb_check_call(plan, good, 5, 33, out, 33), "leaves the arena");
	ok &= expect("an offset leaves the arena", bn::cb_check_call(plan, good, 5, 16, out, 16), "leaves the arena");
	reset();
	r[2] = 0;
	ok &= expect("null row", bn::cb_check_call(plan, r, 5, len, out, len), "null or misaligned row");
	reset();
	r[3] = good[3] + 4;
	ok &= expect("misaligned row", bn::cb_check_call(plan, r, 5, len, out, len), "null or misaligned row");
	reset();
	r[0] = out + 16 * 23; // the last element of job 0's output
	ok &= expect("an output overlaps a row of its own job", bn::cb_check_call(plan, r, 5, len, out, len), "overlaps a row");
	reset();
	r[4] = out + 16 * 16; // job 1's row (2 elements) on job 0's output
	ok &= expect("an output overlaps a row of another job", bn::cb_check_call(plan, r, 5, len, out, len), "overlaps a row");
	reset();
	r[2] = out + 16 * 9; // 8 elements from 9: ends inside job 0's output
	ok &= expect("a row's tail overlaps an output", bn::cb_check_call(plan, r, 5, len, out, len), "overlaps a row");
	reset();
	r[2] = out + 16 * 8; // 8 elements from 8: ends where job 0's output starts
	g_cases++;
	if (const char *why = bn::cb_check_call(plan, r, 5, len, out, len)) {
		std::printf("FAIL a row that ends where an output starts is rejected: %s\n", why);
		ok = false;
	}
	return ok;
}

int main()
{
	bool ok = true;
	const Member b8_mixed = products(2, {0, 3}, 3), b32 = products(1, {5, 5}, 5), b128 = products(1, {3, 7}, 7), pack{{VAR(0), CST(2), MUL(0, 1), VAR(1), ADD(2, 3)}, {0, 3}, 3};
	const Member cst{{CST(5)}, {}, 3}, pw{{VAR(0), POW(0, 5)}, {4}, 4}, ident{{VAR(0)}, {0}, 5};
	// 1, 2, 3 and 33 jobs: bisection over counts that are no powers of two; below, at and above one unit
	ok &= run_batch("one job", {kSelect}, {{0, 10, -1}}, 1);
	ok &= run_batch("two jobs", {kSelect, b8_mixed}, {{0, 17, -1}, {1, 8, -1}}, 2);
	ok &= run_batch("three jobs", {kSelect, b8_mixed, b32}, {{1, 4, -1}, {0, 18, -1}, {2, 12, -1}}, 3);
	{
		std::vector<JobSpec> specs;
		for (uint32_t j = 0; j < 33; j++) specs.push_back(JobSpec{0, j % 5 == 3 ? 18u : j % 3 == 1 ? 17u : 8u + j % 3, -1});
		ok &= run_batch("33 jobs of one program", {kSelect}, specs, 1);
	}
	// 1, 2, 1024 and 2048 output elements in one batch, not in ascending order
	ok &= run_batch("sizes at B1", {kSelect}, {{0, 17, -1}, {0, 7, -1}, {0, 18, -1}, {0, 8, -1}}, 1);
	ok &= run_batch("sizes at B8 and B128", {b8_mixed, b128}, {{0, 14, -1}, {1, 0, -1}, {0, 15, -1}, {1, 1, -1}, {1, 10, -1}, {1, 11, -1}, {0, 4, -1}, {0, 5, -1}}, 2);
	// classes mixed: 2, 4 (Q = 4), 5, 8 (Q = 2), 9, 16 (Q = 1) live slots
	{
		const std::vector<uint32_t> slots = {2, 4, 5, 8, 9, 16};
		std::vector<Member> ms;
		for (size_t i = 0; i < slots.size(); i++) ms.push_back(products(slots[i] - 1, i % 2 ? std::vector<uint32_t>{0, 3} : std::vector<uint32_t>{3, 0, 3}, i == 5 ? 4 : 3));
		ok &= run_batch("classes mixed", ms, {{5, 13, -1}, {0, 4, -1}, {3, 14, -1}, {1, 15, -1}, {4, 5, -1}, {2, 14, -1}, {0, 15, -1}}, 6, slots);
		ok &= run_batch("a 16-slot job among two-slot jobs", {ms[0], ms[5]}, {{0, 14, -1}, {1, 4, -1}, {0, 15, -1}}, 2, {2, 16});
		ok &= run_batch("classes mixed, B1", {products(3, {0}, 0), products(7, {0}, 0), products(15, {0}, 0)}, {{2, 8, -1}, {0, 18, -1}, {1, 17, -1}, {2, 17, -1}}, 3, {4, 8, 16});
	}
	// duplicate programs collapse: members compiled separately from the same steps, and one that differs in a level only
	ok &= run_batch("duplicates", {kSelect, kSelect, b8_mixed, kSelect, b8_mixed}, {{0, 9, -1}, {1, 10, -1}, {2, 9, -1}, {3, 17, -1}, {4, 5, -1}}, 2);
	ok &= run_batch("same steps, other levels", {products(1, {0, 3}, 3), products(1, {3, 3}, 3), products(1, {3, 3}, 4)}, {{0, 9, -1}, {1, 9, -1}, {2, 9, -1}}, 3);
	// a job without inputs, an identity (no ops), a POW, constants at their own offsets
	ok &= run_batch("a constant", {cst}, {{0, 4, -1}}, 1);
	ok &= run_batch("a constant among others", {pack, cst, pw, ident}, {{0, 9, -1}, {1, 15, -1}, {2, 8, -1}, {3, 7, -1}, {0, 14, -1}, {1, 4, -1}}, 4);
	// one row used by several jobs
	ok &= run_batch("shared rows", {kSelect, products(1, {0, 0}, 0)}, {{0, 10, -1}, {0, 10, 0}, {1, 10, 0}, {0, 17, -1}, {1, 17, 3}}, 2);
	ok &= rejections();
	if (!ok) return 1;
	std::printf("compose_batch_check ok: %d cases\n", g_cases);
	return 0;
}
