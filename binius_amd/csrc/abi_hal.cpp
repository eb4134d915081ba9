// binius_amd/csrc/abi_hal.cpp -- extern "C" entry points of the OLD hardware abstraction layer
// (binius_hal::ComputationBackend, crates/hal/src/backend.rs:35-84) for device-resident multilinears:
// bn_hal_round_evals = sumcheck_compute_round_evals (crates/hal/src/sumcheck_round_calculation.rs:45-330),
// bn_hal_fold_multilinear = one multilinear of sumcheck_fold_multilinears (crates/hal/src/sumcheck_folding.rs:16-237).
//
// Routing: compositions that are sums of monomials of at most three FULL multilinears (two next to an equality-indicator
// table), evaluated at X = 1 and X = infinity in High-to-Low order -- the bivariate products of the v2 provers, the
// zerocheck-style constraints a * b + c -- are sums of what the ComputeLayer path evaluates and run on its kernels, one
// pass per distinct monomial (two factors: matrix-core Gram kernels from 2^17 points, 9-lane kernels below; more: the
// bit-sliced product-sum kernel).  Everything else (more evaluation points, Low-to-High order, truncated multilinears,
// larger compositions) runs the general kernels of kernels_hal.hip.  Transparent multilinears are first partially
// evaluated at the tensor query into context scratch (evaluate_partial_low / _high = the fold_right / fold_left
// kernels): the reference does the same thing subcube by subcube to save memory
// (sumcheck_round_calculation.rs:404-418, 496-518).
#include <algorithm>
#include <chrono>
#include <memory>
#include <map>

#include "abi_common.hpp"
#include "hostmul.hpp"

namespace {

// An ArithCircuit as a sum of monomials  coeff * prod(vars)  over GF(2^128) (variables may repeat: a^2 * b is the
// multiset {a, a, b}).  Empty result = too large for the routed path (more than kMaxTerms monomials / degree > 3 / a
// power above 3): the caller falls back to the interpreter kernel.
typedef bn_expr::monomial monomial;
constexpr size_t kMaxTerms = 12;
// (flat: a polynomial is a short vector of terms kept sorted by their variables -- a constraint set compiles two hundred of these
// per prove, and ordered maps of vectors cost a prove's zerocheck milliseconds of allocations)
bool expand_poly(const bn_expr *e, std::vector<monomial> &out)
{
	struct term {
		uint32_t n = 0, v[3] = {0, 0, 0};
		f128 c{0, 0};
	};
	typedef std::vector<term> poly;
	auto less = [](const term &x, const term &y) {
		if (x.n != y.n) return x.n < y.n;
		for (uint32_t i = 0; i < x.n; i++)
			if (x.v[i] != y.v[i]) return x.v[i] < y.v[i];
		return false;
	};
	auto same = [](const term &x, const term &y) { return x.n == y.n && (x.n < 1 || x.v[0] == y.v[0]) && (x.n < 2 || x.v[1] == y.v[1]) && (x.n < 3 || x.v[2] == y.v[2]); };
	auto add_term = [&](poly &p, const term &t) {
		if (t.c == bn::f128_zero()) return;
		for (size_t i = 0; i < p.size(); i++)
			if (same(p[i], t)) {
				p[i].c ^= t.c;
				if (p[i].c == bn::f128_zero()) p.erase(p.begin() + (long)i);
				return;
			}
		p.push_back(t);
	};
	auto mul = [&](const poly &x, const poly &y, poly &r) -> bool {
		for (const term &tx : x)
			for (const term &ty : y) {
				if (tx.n + ty.n > 3) return false;
				term t;
				t.n = tx.n + ty.n;
				for (uint32_t i = 0; i < tx.n; i++) t.v[i] = tx.v[i];
				for (uint32_t i = 0; i < ty.n; i++) t.v[tx.n + i] = ty.v[i];
				std::sort(t.v, t.v + t.n);
				t.c = (tx.c == bn::f128_one()) ? ty.c : (ty.c == bn::f128_one()) ? tx.c : bn::mul_host(tx.c, ty.c);
				add_term(r, t);
			}
		return r.size() <= 4 * kMaxTerms;
	};
	std::vector<poly> val(e->steps.size());
	for (size_t i = 0; i < e->steps.size(); i++) {
		const bn_step &st = e->steps[i];
		poly &r = val[i];
		switch (st.kind) {
		case BN_STEP_VAR: {
			term t;
			t.n = 1;
			t.v[0] = st.a;
			t.c = bn::f128_one();
			r.push_back(t);
			break;
		}
		case BN_STEP_CONST: {
			term t;
			t.c = f128{st.cst.lo, st.cst.hi};
			add_term(r, t);
			break;
		}
		case BN_STEP_ADD:
			if (st.a >= i || st.b >= i) return false;
			r = val[st.a];
			for (const term &t : val[st.b]) add_term(r, t);
			break;
		case BN_STEP_MUL:
			if (st.a >= i || st.b >= i) return false;
			if (!mul(val[st.a], val[st.b], r)) return false;
			break;
		case BN_STEP_POW: {
			if (st.a >= i || st.b > 3) return false;
			poly acc;
			term one;
			one.c = bn::f128_one();
			acc.push_back(one);
			for (uint64_t k = 0; k < st.b; k++) {
				poly nxt;
				if (!mul(acc, val[st.a], nxt)) return false;
				acc.swap(nxt);
			}
			r = acc;
			break;
		}
		default: return false;
		}
	}
	out.clear();
	if (e->steps.empty()) return true;
	poly fin = val.back();
	std::sort(fin.begin(), fin.end(), less); // (the order the callers' job lists were built in: shorter monomials first, then by variable)
	for (const term &t : fin) out.push_back(monomial{std::vector<uint32_t>(t.v, t.v + t.n), t.c});
	return out.size() <= kMaxTerms;
}

// Transparent multilinear -> 2^n_vars large-field values at `dst` under the query
int materialise(bn_ctx *ctx, uint32_t order, uint32_t n_vars, const bn_hal_multilinear &ml, const void *d_query, uint32_t query_vars, void *d_one,
                void *dst)
{
	BN_REQUIRE(valid_tower_level(ml.tower_level), "unsupported value of tower_level");
	BN_REQUIRE(ml.n_vars_ml == n_vars + query_vars, "transparent multilinear: n_vars_ml must equal n_vars + query variables");
	BN_REQUIRE(ml.len << (7 - ml.tower_level) == (uint64_t)1 << ml.n_vars_ml, "transparent multilinear: packed length does not match n_vars_ml");
	BN_REQUIRE(query_vars == 0 || d_query, "tensor query missing while a multilinear is still transparent");
	const void *q = query_vars ? d_query : d_one;
	const uint64_t q_len = (uint64_t)1 << query_vars, out_len = (uint64_t)1 << n_vars;
	if (order == BN_ORDER_LOW_TO_HIGH)
		BN_HIP(bn::launch_fold_right(ctx->stream, ctx->n_cu, ml.d_evals, ml.tower_level, q, q_len, dst, out_len));
	else
		BN_HIP(bn::launch_fold_left(ctx->stream, ctx->n_cu, ml.d_evals, ml.tower_level, q, q_len, dst, out_len));
	return BN_OK;
}

// the expansion of a compiled circuit, computed once per bn_expr (nullptr: not a polynomial the routed paths take)
const std::vector<monomial> *poly_of(const bn_expr *e)
{
	if (e->poly_state == 0) e->poly_state = expand_poly(e, e->poly) ? 1 : 2;
	return e->poly_state == 1 ? &e->poly : nullptr;
}

// all-ones | all-zeros tables of at least `half` elements each (ones at hal_const, zeros hal_const_half elements behind it): filled
// once for the largest size asked for so far and kept in the context -- the rounds of a sumcheck ask for halving sizes
int hal_const_tables(bn_ctx *ctx, uint64_t half)
{
	if (ctx->hal_const && ctx->hal_const_half >= half) return BN_OK;
	if (ctx->hal_const) {
		BN_HIP(hipStreamSynchronize(ctx->stream));
		BN_HIP(hipFree(ctx->hal_const));
		ctx->hal_const = nullptr;
		ctx->hal_const_half = 0;
	}
	if (hipMalloc(&ctx->hal_const, 2 * half * sizeof(f128)) != hipSuccess) {
		(void)hipGetLastError();
		ctx->hal_const = nullptr;
		return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (constant tables of the round evaluation)");
	}
	BN_HIP(bn::launch_fill(ctx->stream, ctx->hal_const, half, bn::f128_one()));
	BN_HIP(hipMemsetAsync((char *)ctx->hal_const + half * sizeof(f128), 0, half * sizeof(f128), ctx->stream));
	ctx->hal_const_half = half;
	return BN_OK;
}

// ---- a constraint set's zerocheck in TWO launches per round --------------------------------------------------------------------
// The reference hands sumcheck_compute_round_evals one equality-indicator evaluator per constraint over every column of the table
// (core/src/constraint_system/prove.rs:431-505; keccak: 100 constraints of degree 2 over 204 columns), evaluation points 1 and
// infinity, High-to-Low, every multilinear Folded and full.  With every composition a sum of monomials of at most two columns,
//     S_e(1) = sum_t coeff_t <eq, prod(vars_t)(upper halves)>,   S_e(inf) = sum_t' coeff_t' <eq, prod(vars_t')(lower + upper halves)>
// and every DISTINCT monomial of the whole set is a job of ONE launch of the claim groups' kernel (kernels_group.hip):
//     {u, w}   an evaluate job (kind 1: both sums at once) over (E_lo | E_hi) and (w_lo | w_hi), with E = eq (.) u on both halves of u
//              -- eq (.) (u_lo + u_hi) = E_lo + E_hi, so its sum at infinity is the three-factor sum the evaluator asks for;
//     {v}, {}  plain inner products with the indicator, two to a job (kind 2): <v_hi, eq> for the sum at 1 -- and <v_lo, eq> beside
//              it only where some composition's form at infinity holds the monomial (a leading form of degree 2 holds none).  The scaled
// columns E are one launch of the batched element-wise product (kernels_mul9.hip k_mul9_jobs) in front; which column of a product
// is scaled is a greedy vertex cover of the products' graph (keccak's chi rows are five-cycles: three scaled columns per row
// instead of five).  The coefficients are applied to the 16-byte sums on the host.  The plan (monomials, cover, terms per
// evaluator) is kept while the same compiled compositions come back.
struct eq_set_plan {
	std::vector<const bn_expr *> key; // (composition, composition_at_infinity) per evaluator
	uint64_t epoch = 0;               // bn::expr_epoch() when the plan was made: no expression has been freed since
	uint32_t n_mls = 0;
	struct mono {
		int u = -1, w = -1; // {}: -1, -1; {v}: v, -1; {u, w}: u = the scaled column
		bool at_inf = false; // some evaluator's form at infinity holds it
		uint32_t s1 = 0, s_lo = 0; // where its sums come back: products: s1 = at 1, s1 + 1 = at infinity; others: s1 = <hi, eq>, s_lo = <lo, eq> (at_inf only)
	};
	struct row_product { // a kind-2 entry: <column half, eq>
		int v;           // the column (-1: the all-ones row)
		bool upper;
		uint32_t slot;
	};
	std::vector<uint32_t> products; // monos with two columns, in job order
	std::vector<row_product> rows;
	uint32_t n_slots = 0;
	std::vector<mono> monos;
	std::vector<uint32_t> scaled; // columns with an E array, in E order
	std::vector<int> e_of;        // column -> its E index (-1: none)
	struct term {
		uint32_t mono;
		f128 coeff;
	};
	std::vector<std::vector<term>> t1, tinf; // per evaluator
};
constexpr uint32_t kEqSetMaxScaled = 256; // (two element-wise jobs each: the pinned table holds 512)
constexpr uint32_t kEqSetMaxMonos = 4096;
constexpr uint32_t kMaxMulJobs = 2 * kEqSetMaxScaled; // the pinned element-wise job table

// the pinned job table of the element-wise launches, allocated on first use (`declined`: no pinned memory -- not this path)
int ensure_mul_jobs(bn_ctx *ctx, int declined)
{
	if (ctx->h_mul_jobs) return BN_OK;
	if (hipHostMalloc(&ctx->h_mul_jobs, kMaxMulJobs * sizeof(bn::mul9_job), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
		(void)hipGetLastError();
		ctx->h_mul_jobs = nullptr;
		return declined;
	}
	BN_HIP(hipHostGetDevicePointer(&ctx->d_mul_jobs, ctx->h_mul_jobs, 0));
	return BN_OK;
}

// ONE launch of the claim groups' kernel over `jobs`, its sums into grp.d_S and from there into the group mailbox (`declined`: the
// kernel does not take the jobs); *seq is what mail_wait waits for
int launch_group_sums(bn_ctx *ctx, const std::vector<bn::group_job> &jobs, uint32_t n_slots, int declined, const char *what, uint64_t *seq)
{
	ctx->mirror.valid = false;
	const hipError_t e = group_launch(ctx, BN_PROF_ROUND_EVAL_MFMA, jobs.data(), (uint32_t)jobs.size(), n_slots, ctx->grp.d_S, ctx->grp.d_gmail, seq);
	if (e == hipSuccess) return BN_OK;
	--ctx->mail_seq;
	(void)hipGetLastError();
	return e == hipErrorNotSupported ? declined : bn::hip_fail(e, what);
}
void read_group_sums(bn_ctx *ctx, f128 *sums, uint32_t n)
{
	for (uint32_t i = 0; i < n; i++) {
		sums[i].lo = __atomic_load_n(&ctx->grp.h_gmail[i].lo, __ATOMIC_RELAXED);
		sums[i].hi = __atomic_load_n(&ctx->grp.h_gmail[i].hi, __ATOMIC_RELAXED);
	}
}

std::shared_ptr<eq_set_plan> make_eq_set_plan(const bn_hal_evaluator *evs, uint32_t n_evs, uint32_t n_mls)
{
	auto pl = std::make_shared<eq_set_plan>();
	pl->n_mls = n_mls;
	pl->epoch = bn::expr_epoch();
	std::map<std::vector<uint32_t>, uint32_t> index;
	pl->t1.resize(n_evs);
	pl->tinf.resize(n_evs);
	for (uint32_t e = 0; e < n_evs; e++) {
		pl->key.push_back(evs[e].composition);
		pl->key.push_back(evs[e].composition_at_infinity);
		for (int which = 0; which < 2; which++) {
			const std::vector<monomial> *p = poly_of(which ? evs[e].composition_at_infinity : evs[e].composition);
			if (!p) return nullptr;
			for (const monomial &t : *p) {
				if (t.vars.size() > 2) return nullptr;
				for (uint32_t v : t.vars)
					if (v >= n_mls) return nullptr;
				auto it = index.find(t.vars);
				if (it == index.end()) {
					if (pl->monos.size() >= kEqSetMaxMonos) return nullptr;
					eq_set_plan::mono m;
					if (t.vars.size() >= 1) m.u = (int)t.vars[0];
					if (t.vars.size() == 2) m.w = (int)t.vars[1];
					it = index.emplace(t.vars, (uint32_t)pl->monos.size()).first;
					pl->monos.push_back(m);
				}
				(which ? pl->tinf[e] : pl->t1[e]).push_back(eq_set_plan::term{it->second, t.coeff});
				if (which) pl->monos[it->second].at_inf = true;
			}
		}
	}
	// which column of every product carries the indicator: the column in the most products not yet covered, again and again
	pl->e_of.assign(n_mls, -1);
	std::vector<char> covered(pl->monos.size(), 0);
	for (;;) {
		std::vector<uint32_t> cnt(n_mls, 0);
		bool any = false;
		for (size_t i = 0; i < pl->monos.size(); i++) {
			const auto &m = pl->monos[i];
			if (m.w < 0 || covered[i]) continue;
			any = true;
			cnt[m.u]++;
			if (m.w != m.u) cnt[m.w]++;
		}
		if (!any) break;
		uint32_t best = 0;
		for (uint32_t v = 1; v < n_mls; v++)
			if (cnt[v] > cnt[best]) best = v;
		if (pl->scaled.size() >= kEqSetMaxScaled) return nullptr;
		pl->e_of[best] = (int)pl->scaled.size();
		pl->scaled.push_back(best);
		for (size_t i = 0; i < pl->monos.size(); i++) {
			auto &m = pl->monos[i];
			if (m.w < 0 || covered[i] || (m.u != (int)best && m.w != (int)best)) continue;
			if (m.w == (int)best) std::swap(m.u, m.w); // u = the scaled one
			covered[i] = 1;
		}
	}
	// the jobs' slots: two per product, one per row product
	for (size_t i = 0; i < pl->monos.size(); i++)
		if (pl->monos[i].w >= 0) {
			pl->monos[i].s1 = pl->n_slots;
			pl->n_slots += 2;
			pl->products.push_back((uint32_t)i);
		}
	for (size_t i = 0; i < pl->monos.size(); i++) {
		auto &m = pl->monos[i];
		if (m.w >= 0) continue;
		m.s1 = pl->n_slots++;
		pl->rows.push_back(eq_set_plan::row_product{m.u, true, m.s1});
		if (m.at_inf && m.u >= 0) { // (the all-ones row is the same at both points)
			m.s_lo = pl->n_slots++;
			pl->rows.push_back(eq_set_plan::row_product{m.u, false, m.s_lo});
		}
	}
	if (pl->n_slots + 1 > (uint32_t)bn::kGroupMaxSlots || pl->products.size() + (pl->rows.size() + 1) / 2 > (size_t)bn::kGroupMaxJobs) return nullptr;
	return pl;
}

constexpr int kEqSetDeclined = -2000; // (internal: not this shape -- the caller goes on with the general code)

// E = eq (.) u on both halves, for every scaled column: one launch (*E stays null where no column is scaled)
int eq_set_scale(bn_ctx *ctx, const eq_set_plan &pl, const bn_hal_multilinear *mls, const void *eq, uint64_t full, char **E)
{
	if (pl.scaled.empty()) return BN_OK;
	const uint64_t half = full >> 1;
	*E = (char *)bn::ctx_scratch(ctx, pl.scaled.size() * full * sizeof(f128));
	if (!*E) return kEqSetDeclined; // (no room: the general code needs less)
	int rc = ensure_mul_jobs(ctx, kEqSetDeclined);
	if (rc) return rc;
	bn::mul9_job *mj = (bn::mul9_job *)ctx->h_mul_jobs;
	for (size_t k = 0; k < pl.scaled.size(); k++) {
		const char *u = (const char *)mls[pl.scaled[k]].d_evals;
		char *out = *E + k * full * sizeof(f128);
		mj[2 * k] = bn::mul9_job{u, eq, out};
		mj[2 * k + 1] = bn::mul9_job{u + half * sizeof(f128), eq, out + half * sizeof(f128)};
	}
	prof_scope ps(ctx, BN_PROF_OTHER);
	BN_HIP(bn::launch_mul9_jobs(ctx->stream, ctx->n_cu, (const bn::mul9_job *)ctx->d_mul_jobs, (uint32_t)(2 * pl.scaled.size()), half));
	return BN_OK;
}

// the jobs of the ONE sums' launch: the products as evaluate jobs, the row products two to a job
std::vector<bn::group_job> eq_set_jobs(bn_ctx *ctx, const eq_set_plan &pl, const bn_hal_multilinear *mls, const void *eq, const char *E, uint64_t full)
{
	const uint64_t half = full >> 1;
	const char *ones = (const char *)ctx->hal_const;
	std::vector<bn::group_job> jobs;
	jobs.reserve(pl.products.size() + (pl.rows.size() + 1) / 2);
	for (uint32_t mi : pl.products) {
		const auto &m = pl.monos[mi];
		bn::group_job j{};
		j.kind = 1;
		j.n = half;
		j.slot = m.s1;
		const char *Ek = E + (size_t)pl.e_of[m.u] * full * sizeof(f128);
		const char *w = (const char *)mls[m.w].d_evals;
		j.x0[0] = Ek;
		j.x1[0] = Ek + half * sizeof(f128);
		j.x0[1] = w;
		j.x1[1] = w + half * sizeof(f128);
		jobs.push_back(j);
	}
	auto row_ptr = [&](const eq_set_plan::row_product &r) -> const char * {
		if (r.v < 0) return ones;
		return (const char *)mls[r.v].d_evals + (r.upper ? half * sizeof(f128) : 0);
	};
	for (size_t q = 0; q < pl.rows.size(); q += 2) {
		// (kind 2 writes S[slot] and S[slot + 1]: the two row products of a job have adjacent slots by construction)
		bn::group_job j{};
		j.kind = 2;
		j.n = half;
		j.slot = pl.rows[q].slot;
		j.x0[0] = row_ptr(pl.rows[q]);
		j.x0[1] = eq;
		if (q + 1 < pl.rows.size()) {
			j.x1[0] = row_ptr(pl.rows[q + 1]);
			j.x1[1] = eq;
		}
		jobs.push_back(j);
	}
	return jobs;
}

// the evaluators' values: coefficient x sum, the sum at 1 or at infinity
void eq_set_values(const eq_set_plan &pl, const bn_hal_evaluator *evs, uint32_t n_evs, const std::vector<f128> &sums, bn_f128 *h_out)
{
	auto sum_at = [&](const eq_set_plan::mono &m, uint32_t p) -> f128 {
		if (p != 2) return sums[m.s1];
		if (m.w >= 0) return sums[m.s1 + 1];
		return m.u >= 0 ? sums[m.s1] ^ sums[m.s_lo] : sums[m.s1]; // <v_lo + v_hi, eq>
	};
	size_t off = 0;
	for (uint32_t e = 0; e < n_evs; e++)
		for (uint32_t p = evs[e].eval_point_start; p < evs[e].eval_point_end; p++, off++) {
			f128 v = bn::f128_zero();
			for (const auto &t : (p == 1 ? pl.t1[e] : pl.tinf[e])) {
				const f128 sv = sum_at(pl.monos[t.mono], p);
				v ^= (t.coeff == bn::f128_one()) ? sv : bn::mul_host(t.coeff, sv);
			}
			h_out[off] = bn_f128{v.lo, v.hi};
		}
}

int round_evals_eq_set(bn_ctx *ctx, uint32_t n_vars, const bn_hal_multilinear *mls, uint32_t n_mls, const bn_hal_evaluator *evs, uint32_t n_evs, bn_f128 *h_out)
{
	const uint64_t full = (uint64_t)1 << n_vars, half = full >> 1;
	const void *eq = n_evs ? evs[0].d_eq_ind : nullptr;
	if (!eq || !ctx->grp.enabled) return kEqSetDeclined;
	// BN_GROUP_PROF=1 (diagnostic): host microseconds of this path by phase, printed every 64 calls
	static thread_local double prof_us[6] = {0, 0, 0, 0, 0, 0};
	static thread_local uint64_t prof_calls = 0;
	auto t_lap = std::chrono::steady_clock::now();
	auto lap = [&](int ph) {
		if (!ctx->grp.prof) return;
		const auto now = std::chrono::steady_clock::now();
		prof_us[ph] += std::chrono::duration<double, std::micro>(now - t_lap).count();
		t_lap = now;
	};
	for (uint32_t k = 0; k < n_mls; k++)
		if (mls[k].kind != BN_HAL_ML_FOLDED || mls[k].len < full || !mls[k].d_evals) return kEqSetDeclined;
	for (uint32_t e = 0; e < n_evs; e++)
		if (evs[e].d_eq_ind != eq || evs[e].eval_point_start < 1 || evs[e].eval_point_end > 3 || !evs[e].composition || !evs[e].composition_at_infinity)
			return kEqSetDeclined;
	// ---- the plan: the last one, if the same compiled compositions came back
	std::shared_ptr<eq_set_plan> pl = std::static_pointer_cast<eq_set_plan>(ctx->hal_set_plan);
	bool same = pl && pl->epoch == bn::expr_epoch() && pl->n_mls == n_mls && pl->key.size() == 2 * (size_t)n_evs;
	for (uint32_t e = 0; e < n_evs && same; e++) same = pl->key[2 * e] == evs[e].composition && pl->key[2 * e + 1] == evs[e].composition_at_infinity;
	if (!same) {
		pl = make_eq_set_plan(evs, n_evs, n_mls);
		ctx->hal_set_plan = pl; // (nullptr: the next call plans again -- and declines again)
		if (!pl) return kEqSetDeclined;
	}
	lap(0);
	int rc = hal_const_tables(ctx, half);
	if (rc) return rc;
	rc = group_res_alloc(ctx);
	if (rc) return rc;
	char *E = nullptr;
	rc = eq_set_scale(ctx, *pl, mls, eq, full, &E);
	if (rc) return rc;
	lap(1);
	std::vector<f128> sums(pl->n_slots);
	const std::vector<bn::group_job> jobs = eq_set_jobs(ctx, *pl, mls, eq, E, full);
	lap(2);
	if (!jobs.empty()) {
		uint64_t seq = 0;
		// (an odd last row product leaves its job's second slot unused: one slot more than the plan counts)
		rc = launch_group_sums(ctx, jobs, pl->n_slots + 1, kEqSetDeclined, "launch_group (constraint set)", &seq);
		if (rc) return rc;
		lap(3);
		rc = mail_wait(ctx, seq);
		if (rc) return rc;
		lap(4);
		read_group_sums(ctx, sums.data(), pl->n_slots);
	}
	eq_set_values(*pl, evs, n_evs, sums, h_out);
	lap(5);
	if (ctx->grp.prof && (++prof_calls & 63) == 0)
		fprintf(stderr, "[bn eq-set prof] %llu calls, host us: plan %.1f, tables + scaling launch %.1f, jobs %.1f, sums launch %.1f, wait %.1f, read + values %.1f\n",
		        (unsigned long long)prof_calls, prof_us[0], prof_us[1], prof_us[2], prof_us[3], prof_us[4], prof_us[5]);
	return BN_OK;
}

// ---- compositions of degree <= 3 at ANY evaluation points: the round polynomial's COEFFICIENTS from bilinear sums ---------------------
// High-to-Low, every multilinear Folded and full: v(X) = v_lo + X dv (dv = v_lo + v_hi), so a monomial's sum over the half cube is a
// polynomial in X whose coefficients are sums of products of HALVES -- no row is ever brought to a domain point z on the device (the
// general code below multiplies every row by z through nibble tables, once per point), and any number of domain points costs the
// same: the 16-byte coefficients meet z on the host.  With [x, y] = sum_i x[i] y[i] over the half cube:
//     {v}        k0 = [v_lo, e]   k1 = [dv, e]                                   (e = the indicator, or the all-ones row)
//     {u, w}     k0 = [u_lo, w_lo]   k2 = [du, dw]   P(1) = [u_hi, w_hi]   k1 = P(1) + k0 + k2
//     {a, b, c}  T0 = a_lo (.) b_lo, T1 = a_hi (.) b_hi, Ti = da (.) db  (element-wise, ONE launch of k_mul9_jobs for every distinct pair
//                of the request: the Karatsuba triple of a (.) b as a polynomial in X)
//                P(1) = [T1, c_hi]   k3 = [Ti, dc]   k0 = [T0, c_lo]   k2 = [Ti, c_hi] + [T0 + T1, dc]   k1 = P(1) + k0 + k2 + k3
// (a (.) b = T0 + X (T0 + T1 + Ti) + X^2 Ti; multiply by c_lo + X dc and collect).  Under an equality indicator the first column of
// every monomial is scaled by it first (both halves: eq (.) du = E_lo + E_hi), as the constraint-set path above does.  Every bracket is
// a job of ONE launch of the claim groups' kernel: [x_hi, y_hi] and [dx, dy] together are an evaluate job (kind 1), a lone bracket half
// a kind-2 job.  So a request is at most three launches (indicator scaling, products, sums) whatever its points and compositions.
// Reference: sumcheck_round_calculation.rs:85-330 evaluates the composition at every point of every vertex pair instead.
constexpr int kCoefDeclined = -2001; // (internal: not this shape)

// One request in coefficient form: what the stages hand to each other.
struct coef_plan {
	struct mono {
		uint32_t n = 0, v[3] = {0, 0, 0};
		bool in1 = false, in_inf = false; // some evaluator wants it at 1 / a domain point; at infinity
		int pair = -1;                    // n = 3: its product triple
		uint32_t s_a = 0, s_b = 0, s_c = 0; // first slots of its jobs
	};
	struct term {
		uint32_t mono;
		f128 coeff;
	};
	struct triple {
		uint32_t x, y; // columns; x is the scaled one under an indicator
		bool t0 = false, t1 = false, ti = false;
	};
	// the request
	bn_ctx *ctx;
	const bn_hal_multilinear *mls;
	uint32_t n_mls;
	const bn_hal_evaluator *evs;
	uint32_t n_evs;
	const void *eq;
	uint64_t half;
	bool has_z;
	// collect_monomials: the distinct monomials of the request, the terms of every evaluator at 1 / a domain point and at infinity
	std::vector<mono> monos;
	std::vector<std::vector<term>> t1, tinf;
	uint32_t deg_max = 0;
	// plan_jobs
	std::vector<int> e_of;        // column -> its scaled copy (-1: none)
	std::vector<uint32_t> scaled; // columns with a scaled copy, in order
	std::vector<triple> pairs;
	bool lone_direct = false;
	uint32_t n_eval_jobs = 0, n_rows = 0, n_lone = 0, rows_base = 0, lone_base = 0, n_slots = 0;
	// launch_products: the scaled columns and the product triples in context scratch
	char *E = nullptr, *T = nullptr;
	// launch_sums
	std::vector<f128> S;

	// does monomial m ride on these jobs of the sums' launch
	bool wants_p1_job(const mono &m) const { return m.n == 3 && m.in1 && has_z; }
	bool wants_inf_job(const mono &m) const { return m.n == 3 && (m.in_inf || (m.in1 && has_z)); }
	uint32_t eval_jobs_of(const mono &m) const { return m.n == 2 ? 1u : (wants_p1_job(m) ? 1u : 0u) + (wants_inf_job(m) ? 1u : 0u); }
	const char *col(uint32_t v) const { return (const char *)mls[v].d_evals; }
	// a monomial's first column: its scaled copy under an indicator
	const char *first_col(uint32_t v) const { return eq ? E + (size_t)e_of[v] * 2 * half * sizeof(f128) : col(v); }
};

// false: a composition is no polynomial of degree <= 3 over the request's multilinears
bool collect_monomials(coef_plan &pl)
{
	std::map<std::vector<uint32_t>, uint32_t> index;
	pl.t1.resize(pl.n_evs);
	pl.tinf.resize(pl.n_evs);
	for (uint32_t e = 0; e < pl.n_evs; e++) {
		const bn_hal_evaluator &ev = pl.evs[e];
		const bool want1 = (ev.eval_point_start <= 1 && ev.eval_point_end > 1) || ev.eval_point_end > 3, want_inf = ev.eval_point_start <= 2 && ev.eval_point_end > 2;
		for (int which = 0; which < 2; which++) {
			if (!(which ? want_inf : want1)) continue;
			const std::vector<monomial> *p = poly_of(which ? ev.composition_at_infinity : ev.composition);
			if (!p) return false;
			for (const monomial &t : *p) {
				if (t.vars.size() > 3) return false;
				for (uint32_t v : t.vars)
					if (v >= pl.n_mls) return false;
				auto it = index.find(t.vars);
				if (it == index.end()) {
					coef_plan::mono m;
					m.n = (uint32_t)t.vars.size();
					for (uint32_t i = 0; i < m.n; i++) m.v[i] = t.vars[i];
					it = index.emplace(t.vars, (uint32_t)pl.monos.size()).first;
					pl.monos.push_back(m);
					pl.deg_max = std::max(pl.deg_max, m.n);
				}
				(which ? pl.tinf[e] : pl.t1[e]).push_back(coef_plan::term{it->second, t.coeff});
				(which ? pl.monos[it->second].in_inf : pl.monos[it->second].in1) = true;
			}
		}
	}
	return true;
}

// scaled columns, product triples, the jobs of the sums' launch and their slots (false: more than the launches carry)
bool plan_jobs(coef_plan &pl)
{
	const bool has_z = pl.has_z;
	// ---- scaled columns (under an indicator: the first column of every monomial of two or three), product triples
	pl.e_of.assign(pl.n_mls, -1);
	std::map<std::pair<uint32_t, uint32_t>, int> pair_index;
	for (coef_plan::mono &m : pl.monos) {
		if (m.n < 2) continue;
		if (pl.eq && pl.e_of[m.v[0]] < 0) {
			pl.e_of[m.v[0]] = (int)pl.scaled.size();
			pl.scaled.push_back(m.v[0]);
		}
		if (m.n == 3) {
			auto key = std::make_pair(m.v[0], m.v[1]);
			auto it = pair_index.find(key);
			if (it == pair_index.end()) {
				it = pair_index.emplace(key, (int)pl.pairs.size()).first;
				pl.pairs.push_back(coef_plan::triple{m.v[0], m.v[1]});
			}
			m.pair = it->second;
			coef_plan::triple &tp = pl.pairs[(size_t)m.pair];
			tp.t1 = tp.t1 || m.in1;
			tp.t0 = tp.t0 || (m.in1 && has_z);
			tp.ti = tp.ti || m.in_inf || (m.in1 && has_z);
		}
	}
	if (2 * pl.scaled.size() + 3 * pl.pairs.size() > kMaxMulJobs) return false;
	// ---- the jobs of the sums' launch and their slots: evaluate jobs (two slots each) first, then the lone brackets two to a job
	for (const coef_plan::mono &m : pl.monos) pl.n_eval_jobs += pl.eval_jobs_of(m);
	// the sum of a lone row without an indicator: at streaming speed into its slot (k_xor_sum), which the sums' launch publishes with
	// its own -- from 2^20 points a bracket with the all-ones row (twice the bytes, and Gram products of ones) costs more than a launch
	// (only where there is a launch for the lone sums to ride on)
	pl.lone_direct = !pl.eq && pl.half >= ((uint64_t)1 << 20) && pl.n_eval_jobs > 0;
	for (const coef_plan::mono &m : pl.monos) {
		if (m.n == 0) pl.n_rows += pl.eq ? 1 : 0;
		if (m.n == 1) (pl.lone_direct ? pl.n_lone : pl.n_rows) += 2;
		if (m.n == 2) pl.n_rows += (has_z && m.in1) ? 1 : 0;
		if (m.n == 3) pl.n_rows += m.in1 ? 1 : 0; // (the sum at 1 without domain points; with them: its k0)
	}
	pl.rows_base = 2 * pl.n_eval_jobs;
	pl.lone_base = pl.rows_base + pl.n_rows + (pl.n_rows & 1);
	pl.n_slots = pl.lone_base + pl.n_lone;
	return pl.n_slots + 1 <= (uint32_t)bn::kGroupMaxSlots && pl.n_eval_jobs + (pl.n_rows + 1) / 2 <= (uint32_t)bn::kGroupMaxJobs;
}

// the request's resources, then the element-wise launches: the indicator's columns, then the product triples
int launch_products(coef_plan &pl)
{
	bn_ctx *ctx = pl.ctx;
	int rc = hal_const_tables(ctx, pl.half);
	if (rc) return rc;
	rc = group_res_alloc(ctx);
	if (rc) return rc;
	if (pl.scaled.empty() && pl.pairs.empty()) return BN_OK;
	const size_t hb = pl.half * sizeof(f128);
	pl.E = (char *)bn::ctx_scratch(ctx, (pl.scaled.size() * 2 + pl.pairs.size() * 3) * hb);
	if (!pl.E) return kCoefDeclined; // (no room: the general code reports it or needs less)
	pl.T = pl.E + pl.scaled.size() * 2 * hb;
	rc = ensure_mul_jobs(ctx, kCoefDeclined);
	if (rc) return rc;
	// (the second launch reads what the first wrote: its jobs sit behind the first launch's in the pinned table, which the first
	// launch may still be reading)
	bn::mul9_job *mj = (bn::mul9_job *)ctx->h_mul_jobs;
	uint32_t n_mj = 0;
	if (!pl.scaled.empty()) {
		for (size_t k = 0; k < pl.scaled.size(); k++) {
			const char *u = pl.col(pl.scaled[k]);
			char *out = pl.E + k * 2 * hb;
			mj[n_mj++] = bn::mul9_job{u, pl.eq, out, nullptr, nullptr};
			mj[n_mj++] = bn::mul9_job{u + hb, pl.eq, out + hb, nullptr, nullptr};
		}
		prof_scope ps(ctx, BN_PROF_OTHER);
		BN_HIP(bn::launch_mul9_jobs(ctx->stream, ctx->n_cu, (const bn::mul9_job *)ctx->d_mul_jobs, n_mj, pl.half));
	}
	if (!pl.pairs.empty()) {
		const uint32_t first = n_mj;
		for (size_t k = 0; k < pl.pairs.size(); k++) {
			const coef_plan::triple &tp = pl.pairs[k];
			const char *x = pl.first_col(tp.x), *y = pl.col(tp.y);
			char *out = pl.T + k * 3 * hb;
			if (tp.t0) mj[n_mj++] = bn::mul9_job{x, y, out, nullptr, nullptr};
			if (tp.t1) mj[n_mj++] = bn::mul9_job{x + hb, y + hb, out + hb, nullptr, nullptr};
			if (tp.ti) mj[n_mj++] = bn::mul9_job{x, y, out + 2 * hb, x + hb, y + hb};
		}
		prof_scope ps(ctx, BN_PROF_OTHER);
		BN_HIP(bn::launch_mul9_jobs(ctx->stream, ctx->n_cu, (const bn::mul9_job *)ctx->d_mul_jobs + first, n_mj - first, pl.half));
	}
	return BN_OK;
}

// The lone slots of grp.d_S between the first streaming sum into them and a successful sums' launch (whose finalize publishes and
// re-zeroes them): the slots are zero between launches, and nothing else re-establishes that -- so whatever returns in between
// zeroes them on the way out.
struct lone_slots {
	bn_ctx *ctx;
	uint32_t base, n = 0;
	~lone_slots()
	{
		if (n) (void)hipMemsetAsync(ctx->grp.d_S + base, 0, n * sizeof(f128), ctx->stream);
	}
};

// every bracket of the request: the lone sums, then ONE launch of the claim groups' kernel; the sums come back in pl.S
int launch_sums(coef_plan &pl)
{
	bn_ctx *ctx = pl.ctx;
	const uint64_t half = pl.half;
	const size_t hb = half * sizeof(f128);
	const bool has_z = pl.has_z;
	const char *ones = (const char *)ctx->hal_const, *zeros = ones + ctx->hal_const_half * sizeof(f128);
	struct bracket {
		const void *x, *y;
	};
	std::vector<bn::group_job> jobs;
	std::vector<bracket> rows;
	uint32_t next_eval = 0;
	lone_slots lone{ctx, pl.lone_base};
	auto eval_job = [&](const void *x_lo, const void *x_hi, const void *y_lo, const void *y_hi) -> uint32_t {
		bn::group_job j{};
		j.kind = 1;
		j.n = half;
		j.slot = 2 * next_eval++;
		j.x0[0] = x_lo;
		j.x1[0] = x_hi;
		j.x0[1] = y_lo;
		j.x1[1] = y_hi;
		jobs.push_back(j);
		return j.slot;
	};
	auto row = [&](const void *x, const void *y) -> uint32_t {
		rows.push_back(bracket{x, y});
		return pl.rows_base + (uint32_t)rows.size() - 1;
	};
	const void *e_row = pl.eq ? pl.eq : (const void *)ones;
	for (coef_plan::mono &m : pl.monos) {
		if (m.n == 0) {
			if (pl.eq) m.s_a = row(ones, pl.eq);
		} else if (m.n == 1) {
			const char *v = pl.col(m.v[0]);
			if (pl.lone_direct) {
				m.s_a = pl.lone_base + lone.n;
				m.s_b = m.s_a + 1;
				lone.n += 2; // (before the launches: a failure of either leaves through the guard)
				prof_scope ps(ctx, BN_PROF_OTHER);
				BN_HIP(bn::launch_xor_sum(ctx->stream, ctx->n_cu, v + hb, half, ctx->grp.d_S + m.s_a));
				BN_HIP(bn::launch_xor_sum(ctx->stream, ctx->n_cu, v, half, ctx->grp.d_S + m.s_b));
			} else {
				m.s_a = row(v + hb, e_row);
				m.s_b = row(v, e_row);
			}
		} else if (m.n == 2) {
			const char *u = pl.first_col(m.v[0]), *w = pl.col(m.v[1]);
			m.s_a = eval_job(u, u + hb, w, w + hb);
			if (has_z && m.in1) m.s_c = row(u, w);
		} else {
			const char *t0 = pl.T + (size_t)m.pair * 3 * hb, *t1p = t0 + hb, *ti = t0 + 2 * hb, *c = pl.col(m.v[2]);
			if (m.in1) m.s_a = has_z ? eval_job(t0, t1p, c, c + hb) : row(t1p, c + hb);
			if (pl.wants_inf_job(m)) m.s_b = eval_job(zeros, ti, c, c + hb);
			if (m.in1 && has_z) m.s_c = row(t0, c);
		}
	}
	for (size_t q = 0; q < rows.size(); q += 2) {
		bn::group_job j{};
		j.kind = 2;
		j.n = half;
		j.slot = pl.rows_base + (uint32_t)q;
		j.x0[0] = rows[q].x;
		j.x0[1] = rows[q].y;
		if (q + 1 < rows.size()) {
			j.x1[0] = rows[q + 1].x;
			j.x1[1] = rows[q + 1].y;
		}
		jobs.push_back(j);
	}
	pl.S.assign(pl.n_slots + 1, bn::f128_zero());
	uint64_t seq = 0;
	int rc = launch_group_sums(ctx, jobs, pl.n_slots + 1, kCoefDeclined, "launch_group (coefficient form)", &seq);
	if (rc) return rc; // (declined: the element-wise launches wrote scratch only, and the lone slots leave through the guard)
	lone.n = 0;        // (the launch's finalize re-zeroes every slot it publishes)
	ctx->grp.launches++;
	ctx->grp.jobs_eval += jobs.size();
	rc = mail_wait(ctx, seq);
	if (rc) return rc;
	read_group_sums(ctx, pl.S.data(), pl.n_slots);
	return BN_OK;
}

// coefficients k0 .. k_deg and P(1) per monomial, then the evaluators' values
void combine(const coef_plan &pl, const bn_f128 *h_points, bn_f128 *h_out)
{
	const std::vector<f128> &S = pl.S;
	const bool has_z = pl.has_z;
	struct coefs {
		f128 k[4], p1;
	};
	std::vector<coefs> cf(pl.monos.size());
	for (size_t i = 0; i < pl.monos.size(); i++) {
		const coef_plan::mono &m = pl.monos[i];
		coefs &c = cf[i];
		for (auto &x : c.k) x = bn::f128_zero();
		c.p1 = bn::f128_zero();
		if (m.n == 0) {
			if (pl.eq) c.k[0] = c.p1 = S[m.s_a];
		} else if (m.n == 1) {
			c.p1 = S[m.s_a];
			c.k[0] = S[m.s_b];
			c.k[1] = S[m.s_a] ^ S[m.s_b];
		} else if (m.n == 2) {
			c.p1 = S[m.s_a];
			c.k[2] = S[m.s_a + 1];
			if (has_z && m.in1) {
				c.k[0] = S[m.s_c];
				c.k[1] = c.p1 ^ c.k[0] ^ c.k[2];
			}
		} else {
			if (m.in1) c.p1 = S[m.s_a];
			if (pl.wants_inf_job(m)) c.k[3] = S[m.s_b + 1];
			if (m.in1 && has_z) {
				c.k[0] = S[m.s_c];
				c.k[2] = S[m.s_b] ^ S[m.s_a + 1];
				c.k[1] = c.p1 ^ c.k[0] ^ c.k[2] ^ c.k[3];
			}
		}
	}
	auto scaled = [](const f128 &coeff, const f128 &v) { return (coeff == bn::f128_one()) ? v : bn::mul_host(coeff, v); };
	size_t off = 0;
	for (uint32_t e = 0; e < pl.n_evs; e++)
		for (uint32_t p = pl.evs[e].eval_point_start; p < pl.evs[e].eval_point_end; p++, off++) {
			f128 v = bn::f128_zero();
			if (p == 2) {
				for (const coef_plan::term &t : pl.tinf[e]) v ^= scaled(t.coeff, cf[t.mono].k[pl.monos[t.mono].n]);
			} else if (p == 1) {
				for (const coef_plan::term &t : pl.t1[e]) v ^= scaled(t.coeff, cf[t.mono].p1);
			} else {
				// Horner in z over the coefficient sums of the whole composition (coefficients first: four products per point)
				f128 K[4] = {bn::f128_zero(), bn::f128_zero(), bn::f128_zero(), bn::f128_zero()};
				for (const coef_plan::term &t : pl.t1[e])
					for (uint32_t d = 0; d <= pl.monos[t.mono].n; d++) K[d] ^= scaled(t.coeff, cf[t.mono].k[d]);
				const f128 z = to_f(&h_points[p - 3]);
				v = K[3];
				for (int d = 2; d >= 0; d--) v = bn::mul_host(v, z) ^ K[d];
			}
			h_out[off] = bn_f128{v.lo, v.hi};
		}
}

int round_evals_coef(bn_ctx *ctx, uint32_t n_vars, const bn_hal_multilinear *mls, uint32_t n_mls, const bn_hal_evaluator *evs, uint32_t n_evs, const bn_f128 *h_points,
                     uint32_t n_points, bn_f128 *h_out)
{
	if (!ctx->grp.enabled || n_vars < 2 || n_evs == 0) return kCoefDeclined;
	const uint64_t full = (uint64_t)1 << n_vars, half = full >> 1;
	for (uint32_t k = 0; k < n_mls; k++)
		if (mls[k].kind != BN_HAL_ML_FOLDED || mls[k].len < full || !mls[k].d_evals) return kCoefDeclined;
	const void *eq = evs[0].d_eq_ind;
	uint32_t pt_hi = 0, total = 0;
	for (uint32_t e = 0; e < n_evs; e++) {
		if (evs[e].d_eq_ind != eq || !evs[e].composition || !evs[e].composition_at_infinity || evs[e].eval_point_start < 1 || evs[e].eval_point_start > evs[e].eval_point_end)
			return kCoefDeclined;
		if (evs[e].composition->n_vars > n_mls || evs[e].composition_at_infinity->n_vars > n_mls) return kCoefDeclined;
		pt_hi = std::max(pt_hi, evs[e].eval_point_end);
		total += evs[e].eval_point_end - evs[e].eval_point_start;
	}
	if (n_points != (pt_hi > 3 ? pt_hi - 3 : 0) || (n_points && !h_points) || total == 0) return kCoefDeclined; // (the general code reports the error)
	coef_plan pl{};
	pl.ctx = ctx;
	pl.mls = mls;
	pl.n_mls = n_mls;
	pl.evs = evs;
	pl.n_evs = n_evs;
	pl.eq = eq;
	pl.half = half;
	pl.has_z = pt_hi > 3;
	if (!collect_monomials(pl)) return kCoefDeclined;
	// (points 1 and infinity of compositions of degree <= 2 are what the routed code and the constraint-set path above are tuned for)
	if (!pl.has_z && pl.deg_max < 3) return kCoefDeclined;
	if (!plan_jobs(pl)) return kCoefDeclined;
	if (pl.n_eval_jobs + pl.n_rows == 0) { // (constants without an indicator: every sum over the half cube is zero)
		for (uint32_t i = 0; i < total; i++) h_out[i] = bn_f128{0, 0};
		return BN_OK;
	}
	int rc = launch_products(pl);
	if (rc) return rc;
	rc = launch_sums(pl);
	if (rc) return rc;
	combine(pl, h_points, h_out);
	return BN_OK;
}

// The checks bn_hal_round_evals makes of its evaluators, in the order they fire, and the range of points they ask for.  one_pass: the
// request runs as one pass of the general code (a wide one is dealt out to parts, each of which comes back here as a pass).
struct point_range {
	uint32_t lo = 0, hi = 0, total = 0;
};
int validate_evaluators(const bn_hal_evaluator *evs, uint32_t n_evs, uint32_t n_mls, const bn_f128 *h_points, uint32_t n_points, bool one_pass, point_range &pr)
{
	pr = point_range{};
	for (uint32_t e = 0; e < n_evs; e++) {
		BN_REQUIRE(evs[e].composition && evs[e].composition_at_infinity, "evaluator without a composition");
		BN_REQUIRE(evs[e].eval_point_start <= evs[e].eval_point_end, "empty evaluation point range");
		BN_REQUIRE(evs[e].composition->n_vars <= n_mls && evs[e].composition_at_infinity->n_vars <= n_mls,
		           "composition uses more variables than there are multilinears");
		if (one_pass) BN_REQUIRE(evs[e].composition->steps.size() <= 64 && evs[e].composition_at_infinity->steps.size() <= 64, "composition too large");
		if (e == 0 || evs[e].eval_point_start < pr.lo) pr.lo = evs[e].eval_point_start;
		if (e == 0 || evs[e].eval_point_end > pr.hi) pr.hi = evs[e].eval_point_end;
		pr.total += evs[e].eval_point_end - evs[e].eval_point_start;
	}
	// Error::IncorrectNontrivialEvalPointsLength (sumcheck_round_calculation.rs:121-125)
	BN_REQUIRE(n_points == (pr.hi > 3 ? pr.hi - 3 : 0), "nontrivial evaluation points: incorrect length");
	if (!one_pass) return BN_OK;
	BN_REQUIRE(n_points <= (uint32_t)bn::kHalMaxPts && pr.total <= 64, "too many evaluation points");
	BN_REQUIRE(n_points == 0 || h_points, "null argument");
	return BN_OK;
}

// A request wider than one pass of the code below carries (a constraint set's zerocheck: one evaluator per constraint over every
// column of the table, core/src/constraint_system/prove.rs:431-505 -- keccak: a hundred compositions over two hundred
// multilinears, each composition reading four or five of them): the evaluators are dealt out, in order, to parts of at most
// kHalMaxEv evaluators that together read at most kHalMaxMl multilinears and ask for at most 32 values; every part is the same call
// with its compositions' variables renumbered to the multilinears it reads.  The results are those of the whole: an evaluator's
// values depend on nothing but its own compositions and multilinears (sumcheck_round_calculation.rs:85-330).
int round_evals_in_parts(bn_ctx *ctx, uint32_t order, uint32_t n_vars, const void *d_tensor_query, uint32_t query_vars, const bn_hal_multilinear *mls, uint32_t n_mls,
                         const bn_hal_evaluator *evs, uint32_t n_evs, const bn_f128 *h_points, uint32_t n_points, bn_f128 *h_out)
{
	point_range all;
	const int rc_v = validate_evaluators(evs, n_evs, n_mls, h_points, n_points, /*one_pass=*/false, all);
	if (rc_v) return rc_v;
	std::vector<int> local_of(n_mls, -1);
	size_t out_at = 0;
	uint32_t e0 = 0;
	while (e0 < n_evs) {
		std::vector<uint32_t> used;
		uint32_t e1 = e0, pts = 0, pt_hi = 0;
		while (e1 < n_evs && e1 - e0 < (uint32_t)bn::kHalMaxEv) {
			std::vector<uint32_t> fresh;
			for (const bn_expr *c : {(const bn_expr *)evs[e1].composition, (const bn_expr *)evs[e1].composition_at_infinity})
				for (const bn_step &st : c->steps)
					if (st.kind == BN_STEP_VAR && local_of[st.a] < 0 && std::find(fresh.begin(), fresh.end(), st.a) == fresh.end()) fresh.push_back(st.a);
			const uint32_t cnt = evs[e1].eval_point_end - evs[e1].eval_point_start;
			const bool fits = used.size() + fresh.size() <= (size_t)bn::kHalMaxMl && pts + cnt <= 32;
			if (!fits && e1 > e0) break;
			BN_REQUIRE(fits, "one evaluator reads more multilinears or asks for more values than a pass carries");
			for (uint32_t v : fresh) {
				local_of[v] = (int)used.size();
				used.push_back(v);
			}
			pts += cnt;
			if (evs[e1].eval_point_end > pt_hi) pt_hi = evs[e1].eval_point_end;
			e1++;
		}
		std::vector<bn_hal_multilinear> part_mls;
		for (uint32_t v : used) part_mls.push_back(mls[v]);
		std::vector<bn_expr *> owned;
		std::vector<bn_hal_evaluator> part_evs;
		int rc = BN_OK;
		for (uint32_t e = e0; e < e1 && !rc; e++) {
			bn_hal_evaluator pe = evs[e];
			for (int which = 0; which < 2 && !rc; which++) {
				const bn_expr *c = which ? evs[e].composition_at_infinity : evs[e].composition;
				std::vector<bn_step> steps = c->steps;
				for (bn_step &st : steps)
					if (st.kind == BN_STEP_VAR) st.a = (uint32_t)local_of[st.a];
				bn_expr *re = nullptr;
				rc = bn_expr_compile(ctx, steps.data(), steps.size(), &re);
				if (rc) break;
				owned.push_back(re);
				(which ? pe.composition_at_infinity : pe.composition) = re;
			}
			part_evs.push_back(pe);
		}
		std::vector<bn_f128> part_out(pts ? pts : 1);
		if (!rc)
			rc = bn_hal_round_evals(ctx, order, n_vars, d_tensor_query, query_vars, part_mls.data(), (uint32_t)part_mls.size(), part_evs.data(), (uint32_t)part_evs.size(),
			                        h_points, pt_hi > 3 ? pt_hi - 3 : 0, part_out.data());
		for (bn_expr *x : owned) bn_expr_free(x);
		if (rc) return rc;
		for (uint32_t i = 0; i < pts; i++) h_out[out_at + i] = part_out[i];
		out_at += pts;
		for (uint32_t v : used) local_of[v] = -1;
		e0 = e1;
	}
	return BN_OK;
}

// ---- one call of bn_hal_round_evals ---------------------------------------------------------------------------------------------------
// The 64 accumulator slots of a request (slots 0..63 of the result area): zero when a route starts, zero again -- and known to be,
// ctx->s_clean -- when the request has been answered.  An error return in between leaves s_clean false: whoever needs the slots next
// zeroes them first.
struct acc_scope {
	bn_ctx *ctx;
	int begin()
	{
		ctx->s_clean = false;
		BN_HIP(hipMemsetAsync(ctx->d_result, 0, 64 * sizeof(f128), ctx->stream));
		return BN_OK;
	}
	// a route that leaves the slots to code with its own account of them (circuit_ip_run): zeroed by begin(), untouched since
	void hand_over_clean() { ctx->s_clean = true; }
	int end()
	{
		BN_HIP(hipMemsetAsync(ctx->d_result, 0, 64 * sizeof(f128), ctx->stream));
		ctx->s_clean = true;
		return BN_OK;
	}
};

// The request, and what the routes share.
struct hal_request {
	bn_ctx *ctx;
	uint32_t order, n_vars;
	const void *d_tensor_query;
	uint32_t query_vars;
	const bn_hal_multilinear *mls;
	uint32_t n_mls;
	const bn_hal_evaluator *evs;
	uint32_t n_evs;
	const bn_f128 *h_points;
	uint32_t n_points;
	bn_f128 *h_out;
	uint64_t full, half;
	point_range pts;      // validate_evaluators: [pts.lo, pts.hi) over all evaluators, pts.total values
	uint32_t n_tr = 0;    // Transparent multilinears
	// plan_scratch: [partial evaluations of the Transparent multilinears | 1 | rows | circuit temporaries]
	bool rows_ok = false; // rows + compiled circuits apply and have their scratch
	bool batch_points = false;
	uint32_t used_mls = 0; // bit k: multilinear k is read by some composition
	char *scr = nullptr;
	size_t tr_elems = 0, row_elems = 0, temp_elems = 0;
	// resolve_multilinears: Transparent ones partially evaluated, truncated ones with their suffix; the domain points
	bn::hal_round_args a{};
	bool all_full = true;
	acc_scope acc;
	f128 *d_acc = nullptr;
	// what this request adds to bn_hal_counters once it has been answered with BN_OK (answered_by)
	uint64_t cnt[BN_HALCNT_N] = {};

	bool l2h() const { return order == BN_ORDER_LOW_TO_HIGH; }
	size_t rows_off() const { return tr_elems * sizeof(f128); }
	size_t temps_off() const { return (tr_elems + row_elems) * sizeof(f128); }
};

// compositions of degree <= 3 over full Folded multilinears at domain points (or of degree 3 at 1 / infinity): the round
// polynomial's coefficients from bilinear sums, at most three launches whatever the width of the request
routed route_coef(hal_request &r)
{
	if (!(r.order == BN_ORDER_HIGH_TO_LOW && r.ctx->hal_coef)) return routed::decline();
	const int rc = round_evals_coef(r.ctx, r.n_vars, r.mls, r.n_mls, r.evs, r.n_evs, r.h_points, r.n_points, r.h_out);
	return rc == kCoefDeclined ? routed::decline() : routed::answer(rc);
}

// the values the evaluators ask for (before validate_evaluators: an inverted range asks for none)
uint32_t values_asked(const hal_request &r)
{
	uint32_t pts = 0;
	for (uint32_t e = 0; e < r.n_evs; e++) pts += r.evs[e].eval_point_end > r.evs[e].eval_point_start ? r.evs[e].eval_point_end - r.evs[e].eval_point_start : 0;
	return pts;
}

// The request has been answered by `route` with `rc`: BN_OK moves the route's counter and what the route noted on its way
// (bn_hal_counters); an error, or a request that asked for no value, moves nothing.
int answered_by(hal_request &r, int route, int rc)
{
	if (rc != BN_OK || values_asked(r) == 0) return rc;
	r.cnt[route] += 1;
	for (int i = 0; i < BN_HALCNT_N; i++) r.ctx->hal_calls[i] += r.cnt[i];
	return rc;
}

// more than one pass of the general code carries
bool is_wide(const hal_request &r)
{
	return r.n_mls > (uint32_t)bn::kHalMaxMl || r.n_evs > (uint32_t)bn::kHalMaxEv || values_asked(r) > 32;
}

// a constraint set's two launches: a wide request, or any request under an indicator
// (a narrow request under an indicator takes the constraint set's two launches too: the monomial route below runs one pass per
// monomial and reads a lone column's lower half beside an all-zeros table -- measured, (a b + c) eq: n = 13 48 -> 39 us,
// n = 20 96 -> 77 us, n = 24 0.62 -> 0.60 ms, where the 2^24 products of the scaling are what is left)
routed route_eq_set(hal_request &r, bool wide)
{
	if (!(wide || (r.n_evs && r.evs[0].d_eq_ind))) return routed::decline();
	if (!(r.order == BN_ORDER_HIGH_TO_LOW && r.n_points == 0 && r.ctx->hal_eq_set)) return routed::decline();
	const int rc = round_evals_eq_set(r.ctx, r.n_vars, r.mls, r.n_mls, r.evs, r.n_evs, r.h_out);
	return rc == kEqSetDeclined ? routed::decline() : routed::answer(rc);
}

routed route_in_parts(hal_request &r, bool wide)
{
	if (!wide) return routed::decline();
	return routed::answer(round_evals_in_parts(r.ctx, r.order, r.n_vars, r.d_tensor_query, r.query_vars, r.mls, r.n_mls, r.evs, r.n_evs, r.h_points, r.n_points, r.h_out));
}

int check_multilinears(hal_request &r)
{
	for (uint32_t k = 0; k < r.n_mls; k++) {
		BN_REQUIRE(r.mls[k].kind == BN_HAL_ML_FOLDED || r.mls[k].kind == BN_HAL_ML_TRANSPARENT, "unknown multilinear kind");
		BN_REQUIRE(r.mls[k].d_evals || r.mls[k].len == 0, "multilinear without evaluations");
		if (r.mls[k].kind == BN_HAL_ML_TRANSPARENT) r.n_tr++;
	}
	return BN_OK;
}

// The plan of "rows + compiled circuits", made before anything is launched so that the context scratch is laid out once:
// [partial evaluations of the Transparent multilinears | 1 | rows | circuit temporaries]
int plan_scratch(hal_request &r)
{
	const bn_hal_evaluator *evs = r.evs;
	r.rows_ok = circuit_multipass_applies(r.ctx, evs[0].composition, r.half) && r.pts.total <= 32;
	// In the launch-bound regime the rows of all evaluation points of a multilinear lie side by side and ONE set of product passes
	// serves every point that shares a composition (all points but infinity); from 2^18 rows on the passes are traffic-bound, the
	// copies that would put the X = 0 / 1 halves beside the other rows cost more than the launches they save, and every point runs
	// its own passes.
	// (measured, a·b·c + a at X = 1, infinity, z at n = 20 -- rows of 8 MiB --: 0.140 ms with the points side by side, 0.187 ms with
	// a product pass per point; at n = 24 the copies of the X = 1 rows cost more than the launches)
	r.batch_points = r.half <= ((uint64_t)1 << 19);
	size_t max_temp_elems = 0; // temporaries of the largest plan, in elements
	for (uint32_t e = 0; e < r.n_evs && r.rows_ok; e++)
		for (const bn_expr *c : {(const bn_expr *)evs[e].composition, (const bn_expr *)evs[e].composition_at_infinity}) {
			for (const bn_step &st : c->steps)
				if (st.kind == BN_STEP_VAR) r.used_mls |= 1u << st.a;
			const int t = circuit_multipass_sum_temps(c, evs[e].d_eq_ind != nullptr);
			if (t < 0) r.rows_ok = false;
			const uint32_t n_b = (r.batch_points && c == evs[e].composition) ? evs[e].eval_point_end - evs[e].eval_point_start : 1;
			// (the final sums of all compositions run in ONE launch at the end, so in the launch-bound regime every composition keeps
			// its own temporaries until then: the sum; at traffic-bound sizes every point's passes run one after the other over the
			// same temporaries: the maximum)
			if (t > 0) max_temp_elems = r.batch_points ? max_temp_elems + (size_t)t * n_b * r.half : std::max(max_temp_elems, (size_t)t * n_b * r.half);
		}
	uint32_t n_used = 0;
	for (uint32_t k = 0; k < r.n_mls; k++) n_used += (r.used_mls >> k) & 1;
	r.tr_elems = r.n_tr ? (size_t)r.n_tr * r.full + 1 : 0;
	r.row_elems = r.rows_ok ? (size_t)(r.pts.hi - r.pts.lo) * n_used * r.half : 0;
	r.temp_elems = r.rows_ok ? max_temp_elems : 0;
	if (r.tr_elems + r.row_elems + r.temp_elems == 0) return BN_OK;
	r.scr = (char *)bn::ctx_scratch(r.ctx, (r.tr_elems + r.row_elems + r.temp_elems) * sizeof(f128));
	if (r.scr) return BN_OK;
	r.rows_ok = false; // (no room for the rows: the interpreter kernel needs none)
	if (r.n_tr) {
		r.scr = (char *)bn::ctx_scratch(r.ctx, r.tr_elems * sizeof(f128));
		if (!r.scr) return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (scratch)");
	}
	return BN_OK;
}

// Transparent multilinears: partial evaluation at the query into scratch; the kernels' view of every multilinear and point
int resolve_multilinears(hal_request &r)
{
	bn_ctx *ctx = r.ctx;
	char *one = r.scr + (size_t)r.n_tr * r.full * sizeof(f128);
	if (r.n_tr) BN_HIP(bn::launch_fill(ctx->stream, one, 1, bn::f128_one()));
	bn::hal_round_args &a = r.a;
	a.n_ml = r.n_mls;
	a.n_ev = r.n_evs;
	a.pt_lo = r.pts.lo;
	a.pt_hi = r.pts.hi;
	a.order = r.order;
	a.n_vars = r.n_vars;
	uint32_t t = 0;
	for (uint32_t k = 0; k < r.n_mls; k++) {
		if (r.mls[k].kind == BN_HAL_ML_TRANSPARENT) {
			void *dst = r.scr + (size_t)t++ * r.full * sizeof(f128);
			int rc = materialise(ctx, r.order, r.n_vars, r.mls[k], r.d_tensor_query, r.query_vars, one, dst);
			if (rc) return rc;
			r.cnt[BN_HALCNT_TRANSPARENT] += 1;
			a.ml[k].evals = (const uint4 *)dst;
			a.ml[k].len = r.full;
			a.ml[k].suffix = bn::f128_zero();
		} else {
			a.ml[k].evals = (const uint4 *)r.mls[k].d_evals;
			a.ml[k].len = r.mls[k].len < r.full ? r.mls[k].len : r.full;
			a.ml[k].suffix = to_f(&r.mls[k].suffix_eval);
			if (a.ml[k].len != r.full) r.all_full = false;
		}
	}
	for (uint32_t p = 0; p < r.n_points; p++) a.pts[p] = to_f(&r.h_points[p]);
	return BN_OK;
}

// ---- the monomial route: full Folded multilinears, High-to-Low, evaluation points 1 and infinity, every composition a
// sum of monomials of at most three multilinears (two next to an equality indicator).  Every DISTINCT monomial
// (x indicator table) is ONE pass of the ComputeLayer's product-sum kernels, which return the sums at both points;
// the coefficients are applied to the 16-byte sums on the host.
struct term_job {
	std::vector<uint32_t> vars;
	const void *eq;
	bool at_inf = false; // some composition's form at infinity holds the monomial
};
struct monomial_plan {
	std::vector<term_job> jobs;
	std::vector<std::vector<monomial>> p1, pinf; // per evaluator
	size_t job_of(const std::vector<uint32_t> &vars, const void *eq)
	{
		for (size_t j = 0; j < jobs.size(); j++)
			if (jobs[j].vars == vars && jobs[j].eq == eq) return j;
		jobs.push_back(term_job{vars, eq, false});
		return jobs.size() - 1;
	}
};

// false: not the routed shape
bool plan_monomials(const hal_request &r, monomial_plan &pl)
{
	// (Low-to-High order: the pairs are interleaved -- the matrix-core kernel reads them with an element stride of two, so the
	// two-factor jobs take the same path from 2^17 points on)
	const bool l2h = r.l2h();
	if (!((!l2h || bn::mfma_applies(r.ctx->n_cu, r.half)) && r.all_full && r.pts.lo >= 1 && r.pts.hi <= 3 && r.n_vars >= 2)) return false;
	pl.p1.resize(r.n_evs);
	pl.pinf.resize(r.n_evs);
	for (uint32_t e = 0; e < r.n_evs; e++) {
		const bn_hal_evaluator &ev = r.evs[e];
		if (!(expand_poly(ev.composition, pl.p1[e]) && expand_poly(ev.composition_at_infinity, pl.pinf[e]))) return false;
		for (const auto *p : {&pl.p1[e], &pl.pinf[e]})
			for (const auto &t : *p) {
				if (t.vars.size() + (ev.d_eq_ind ? 1 : 0) > (l2h ? 2u : 3u)) return false; // (one slot is kept for the all-ones factor)
				const size_t j = pl.job_of(t.vars, ev.d_eq_ind);
				if (p == &pl.pinf[e]) pl.jobs[j].at_inf = true;
			}
		if (pl.jobs.size() > 15) return false;
	}
	return true;
}

// the pass of one monomial: (S_1, S_inf) into d_out[0], d_out[1]
int launch_monomial(hal_request &r, const term_job &job, const char *ones, const char *zeros, f128 *d_out)
{
	bn_ctx *ctx = r.ctx;
	const uint64_t half = r.half;
	const bool l2h = r.l2h();
	if (job.vars.empty() && !job.eq) { // constant monomial: both sums are zero (the slots are)
		r.cnt[BN_HALCNT_MONO_CONST] += 1;
		return BN_OK;
	}
	if (!l2h && !job.eq && job.vars.size() == 1 && half >= ((uint64_t)1 << 18)) {
		r.cnt[BN_HALCNT_MONO_XOR_SUM] += job.at_inf ? 3 : 1; // (launches)
		// a lone column: its sums at streaming speed (k_xor_sum) -- as a product with the all-ones table it is a pass over twice
		// the bytes, and over its lower half even where no form at infinity holds it (a b + c at n = 24: 0.31 -> 0.2 ms)
		const char *p = (const char *)r.a.ml[job.vars[0]].evals;
		BN_HIP(bn::launch_xor_sum(ctx->stream, ctx->n_cu, p + half * 16, half, d_out));
		if (job.at_inf) {
			BN_HIP(bn::launch_xor_sum(ctx->stream, ctx->n_cu, p + half * 16, half, d_out + 1));
			BN_HIP(bn::launch_xor_sum(ctx->stream, ctx->n_cu, p, half, d_out + 1));
		}
		return BN_OK;
	}
	const void *hi[4] = {nullptr, nullptr, nullptr, nullptr}, *lo[4] = {nullptr, nullptr, nullptr, nullptr};
	uint32_t k = 0, shift[4] = {0, 0, 0, 0};
	for (uint32_t v : job.vars) {
		const char *p = (const char *)r.a.ml[v].evals;
		hi[k] = l2h ? p + 16 : p + half * 16;
		lo[k] = p;
		shift[k] = l2h ? 1 : 0;
		k++;
	}
	if (job.eq) hi[k++] = job.eq; // (lo = NULL: the same factor at both evaluation points)
	while (k < 2) hi[k++] = ones;
	if (k == 2)
		for (uint32_t f = 0; f < 2; f++)
			if (!lo[f]) lo[f] = zeros;
	r.cnt[l2h ? BN_HALCNT_MONO_STRIDED : k == 2 ? BN_HALCNT_MONO_PRODUCT2 : BN_HALCNT_MONO_PRODUCT3] += 1;
	if (l2h)
		BN_HIP(bn::launch_roundeval_mfma_pair_strided(ctx->stream, ctx->n_cu, hi[0], lo[0], shift[0], hi[1], lo[1], shift[1], half, d_out));
	else
		BN_HIP(roundeval_product_routed_pub(ctx, /*scratch_free=*/r.n_tr == 0, hi, lo, k, half, d_out)); // (a * b * eq: routed from 2^20 points)
	return BN_OK;
}

routed route_monomials(hal_request &r)
{
	monomial_plan pl;
	if (!plan_monomials(r, pl)) return routed::decline();
	// A monomial with fewer than two factors is padded with an all-ones table (sum of v = sum of v * 1), and a
	// two-factor job one of whose factors is the same at both points (the indicator, the ones) gets an all-zeros
	// table as that factor's partner, (f + 0) = f: it then has the shape of the bivariate round evaluation and runs on
	// the matrix cores instead of the generic product-sum kernel.
	// The tables are filled once per size and kept in the context (refilling them on every call wrote as many bytes
	// as the job reads).  A monomial without any factor and without an indicator is a constant: its sum over the
	// 2^(n_vars - 1) >= 2 points of the half cube is zero in characteristic 2 -- no pass at all.
	bool need_tables = false;
	for (const auto &j : pl.jobs)
		if (!(j.vars.empty() && !j.eq) && j.vars.size() + (j.eq ? 1 : 0) <= 2 && (j.eq || j.vars.size() < 2)) need_tables = true;
	const char *ones = nullptr, *zeros = nullptr;
	if (need_tables) {
		int rc = hal_const_tables(r.ctx, r.half);
		if (rc) return rc;
		ones = (const char *)r.ctx->hal_const;
		zeros = ones + r.ctx->hal_const_half * sizeof(f128);
	}
	// slots 32 + 2 j, 33 + 2 j: (S_1, S_inf) of job j
	for (size_t j = 0; j < pl.jobs.size(); j++) {
		int rc = launch_monomial(r, pl.jobs[j], ones, zeros, r.d_acc + 32 + 2 * j);
		if (rc) return rc;
	}
	std::vector<f128> sums(2 * pl.jobs.size());
	int rc = publish_vals(r.ctx, r.d_acc + 32, 1, (uint32_t)sums.size(), 0, 0, sums.data()); // (through the mailbox: no copy, no synchronisation)
	if (rc) return rc;
	uint32_t off = 0;
	for (uint32_t e = 0; e < r.n_evs; e++) {
		const bn_hal_evaluator &ev = r.evs[e];
		for (uint32_t p = ev.eval_point_start; p < ev.eval_point_end; p++) {
			f128 v = bn::f128_zero();
			for (const auto &t : (p == 1 ? pl.p1[e] : pl.pinf[e])) v ^= bn::mul_host(t.coeff, sums[2 * pl.job_of(t.vars, ev.d_eq_ind) + (p - 1)]);
			r.h_out[off + (p - ev.eval_point_start)] = bn_f128{v.lo, v.hi};
		}
		off += ev.eval_point_end - ev.eval_point_start;
	}
	return routed::answer(r.acc.end());
}

// ---- everything else at throughput sizes: "rows + compiled circuits".  Every multilinear a composition reads is brought
// to its value at every evaluation point asked for -- e0 / e1 by a gather (nothing at all for a full multilinear in
// High-to-Low order), e0 + e1 for infinity, e0 + z (e0 + e1) through the nibble-table kernel for a domain point; pairs
// as the order says, the constant suffix filled in -- as a plain row of 2^(n_vars - 1) elements, ONCE, whatever the
// number of evaluators.  The composition (at infinity: its leading form) is then compiled into passes of the throughput
// kernels over those rows (abi_circuit.cpp): products on the bit-sliced element-wise kernel, the outermost sum of
// products on the matrix cores.  (The interpreter kernel below walked the cube once per point with a scalar tower
// product per Mul: 170 x slower per point, profiles/r03/hal.jsonl.)
typedef std::vector<std::vector<const void *>> row_table; // [point][multilinear]

// the rows of the request (all of them in as few launches of k_hal_rows as kHalMaxRows allows), and the all-ones row beside them
int build_rows(hal_request &r, row_table &row)
{
	bn_ctx *ctx = r.ctx;
	const uint64_t half = r.half;
	const uint32_t pt_lo = r.pts.lo, pt_hi = r.pts.hi;
	char *rows_base = r.scr + r.rows_off();
	// row storage: multilinear by multilinear, inside a multilinear the evaluation points in the order "all but infinity,
	// ascending; infinity last" -- the points of any evaluator that share its composition are then adjacent
	const uint32_t n_pts = pt_hi - pt_lo;
	auto pos_of = [&](uint32_t p) -> uint32_t {
		if (p == 2) return n_pts - 1;
		return p - pt_lo - ((pt_lo <= 2 && p > 2) ? 1u : 0u);
	};
	row.assign(pt_hi, std::vector<const void *>(r.n_mls, nullptr));
	bn::hal_rows_args ra{};
	ra.order = r.order;
	ra.half = half;
	ra.n_out = half;
	auto flush_rows = [&]() -> int {
		if (ra.n_jobs) {
			BN_HIP(bn::launch_hal_rows(ctx->stream, ctx->n_cu, ra));
			r.cnt[BN_HALCNT_ROWS_LAUNCHES] += 1;
			r.cnt[BN_HALCNT_ROWS_WRITTEN] += ra.n_jobs;
		}
		ra.n_jobs = 0;
		return BN_OK;
	};
	uint32_t ku = 0;
	for (uint32_t k = 0; k < r.n_mls; k++) {
		if (!((r.used_mls >> k) & 1)) continue;
		for (uint32_t p = pt_lo; p < pt_hi; p++) {
			bool wanted = false;
			for (uint32_t e = 0; e < r.n_evs; e++) wanted = wanted || (p >= r.evs[e].eval_point_start && p < r.evs[e].eval_point_end);
			if (!wanted) continue;
			char *dst = rows_base + ((size_t)ku * n_pts + pos_of(p)) * half * sizeof(f128);
			if (!r.batch_points && !r.l2h() && r.a.ml[k].len == r.full && p <= 1) {
				row[p][k] = (const char *)r.a.ml[k].evals + (p ? half * 16 : 0); // the half itself
				r.cnt[BN_HALCNT_ROWS_IN_PLACE] += 1;
				continue;
			}
			// (all the rows of the request in one launch, kernels_hal.hip k_hal_rows)
			auto &jb = ra.jobs[ra.n_jobs++];
			jb.evals = r.a.ml[k].evals;
			jb.out = (uint4 *)dst;
			jb.len = r.a.ml[k].len;
			jb.suffix = r.a.ml[k].suffix;
			jb.z = p >= 3 ? r.a.pts[p - 3] : f128{0, 0};
			jb.point = p;
			row[p][k] = dst;
			if (ra.n_jobs == (uint32_t)bn::kHalMaxRows) {
				int rc = flush_rows();
				if (rc) return rc;
			}
		}
		ku++;
	}
	int rc = flush_rows();
	if (rc) return rc;
	return hal_const_tables(ctx, half); // (the all-ones row: the sum of a lone row is its inner product with it)
}

// launch-bound sizes: the element-wise passes of every composition once for all the points that share it (the rows lie side
// by side), the final sums collected; then ALL sums of the request in one launch
routed route_rows_batched(hal_request &r)
{
	if (!r.rows_ok || !r.batch_points) return routed::decline();
	row_table row;
	int rc = build_rows(r, row);
	if (rc) return rc;
	ip_collector col;
	std::vector<f128> vals(r.pts.total, bn::f128_zero());
	// elements of the temporaries' region handed out so far: every composition keeps its own until the one launch of the sums
	// (plan_scratch laid out the sum of what the compositions need)
	size_t temp_cursor = 0;
	r.acc.hand_over_clean(); // (the accumulator slots were zeroed when the request began, nothing has touched them since)
	uint32_t base = 0;       // the first value of evaluator e
	for (uint32_t e = 0; e < r.n_evs; e++) {
		const bn_hal_evaluator &ev = r.evs[e];
		const uint32_t s0 = ev.eval_point_start, s1 = ev.eval_point_end;
		std::vector<uint32_t> pts; // the points that use ev.composition, in row order
		for (uint32_t p = s0; p < s1; p++)
			if (p != 2) pts.push_back(p);
		auto run = [&](const bn_expr *c, const std::vector<uint32_t> &ps) -> int {
			std::vector<uint32_t> out_index;
			for (uint32_t p : ps) out_index.push_back(base + (p - s0));
			const int t = circuit_multipass_sum_temps(c, ev.d_eq_ind != nullptr);
			int rc_c = circuit_multipass_collect(r.ctx, c, row[ps[0]].data(), r.half, (uint32_t)ps.size(), ev.d_eq_ind, r.temps_off() + temp_cursor * sizeof(f128),
			                                     out_index.data(), col);
			if (rc_c == kCircuitDeclined) return bn::fail(BN_ERR_CORE_LIB, "internal: a planned circuit was declined");
			temp_cursor += t > 0 ? (size_t)t * ps.size() * r.half : 0;
			return rc_c;
		};
		if (!pts.empty()) {
			rc = run(ev.composition, pts);
			if (rc) return rc;
		}
		if (s0 <= 2 && 2 < s1) {
			rc = run(ev.composition_at_infinity, std::vector<uint32_t>{2});
			if (rc) return rc;
		}
		base += s1 - s0;
	}
	rc = circuit_ip_run(r.ctx, col, r.half, vals.data());
	if (rc) return rc;
	for (uint32_t i = 0; i < r.pts.total; i++) r.h_out[i] = bn_f128{vals[i].lo, vals[i].hi};
	return routed::answer(BN_OK);
}

// traffic-bound sizes: every point runs its own passes and product-sum kernels straight into its pair of accumulator
// slots, nothing waits for anything, ONE publish at the end (collecting the final sums for a group launch was measured
// here too: the temporaries then force a launch + wait per composition, 1.30 -> 1.41 - 1.49 ms at n = 24)
routed route_rows_per_point(hal_request &r)
{
	if (!r.rows_ok || r.batch_points) return routed::decline();
	row_table row;
	int rc = build_rows(r, row);
	if (rc) return rc;
	uint32_t idx = 0;
	for (uint32_t e = 0; e < r.n_evs; e++)
		for (uint32_t p = r.evs[e].eval_point_start; p < r.evs[e].eval_point_end; p++, idx++) {
			const bn_expr *c = p == 2 ? r.evs[e].composition_at_infinity : r.evs[e].composition;
			rc = circuit_multipass_sum(r.ctx, c, row[p].data(), r.half, r.evs[e].d_eq_ind, r.d_acc + 2 * idx, r.temps_off());
			if (rc == kCircuitDeclined) return bn::fail(BN_ERR_CORE_LIB, "internal: a planned circuit was declined");
			if (rc) return rc;
		}
	std::vector<f128> direct(r.pts.total);
	rc = publish_vals(r.ctx, r.d_acc, 2, r.pts.total, 1, 2, direct.data()); // value i = slot 2 i + slot 2 i + 1, through the mailbox
	if (rc) return rc;
	for (uint32_t i = 0; i < r.pts.total; i++) r.h_out[i] = bn_f128{direct[i].lo, direct[i].hi};
	return routed::answer(r.acc.end());
}

// the interpreter kernel: any composition at any size in one launch, its values left in the accumulator slots
routed route_interpreter(hal_request &r)
{
	bn::hal_round_args &a = r.a;
	uint32_t off = 0;
	for (uint32_t e = 0; e < r.n_evs; e++) {
		const bn_hal_evaluator &ev = r.evs[e];
		int rc = ensure_d_steps(ev.composition);
		if (rc) return rc;
		rc = ensure_d_steps(ev.composition_at_infinity);
		if (rc) return rc;
		a.ev[e].steps = ev.composition->d_steps;
		a.ev[e].n_steps = (uint32_t)ev.composition->steps.size();
		a.ev[e].steps_inf = ev.composition_at_infinity->d_steps;
		a.ev[e].n_steps_inf = (uint32_t)ev.composition_at_infinity->steps.size();
		a.ev[e].pt_start = ev.eval_point_start;
		a.ev[e].pt_end = ev.eval_point_end;
		a.ev[e].eq = (const uint4 *)ev.d_eq_ind;
		a.ev[e].out_off = off;
		off += ev.eval_point_end - ev.eval_point_start;
	}
	BN_HIP(bn::launch_hal_round_evals(r.ctx->stream, r.ctx->n_cu, a, r.d_acc));
	return routed(routed::launched, hipSuccess);
}

} // namespace

extern "C" {

int bn_hal_round_evals(bn_ctx *ctx, uint32_t order, uint32_t n_vars, const void *d_tensor_query, uint32_t query_vars,
                       const bn_hal_multilinear *mls, uint32_t n_mls, const bn_hal_evaluator *evs, uint32_t n_evs,
                       const bn_f128 *h_points, uint32_t n_points, bn_f128 *h_out)
{
	BN_REQUIRE(ctx && h_out && (mls || n_mls == 0) && (evs || n_evs == 0), "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(order == BN_ORDER_LOW_TO_HIGH || order == BN_ORDER_HIGH_TO_LOW, "unknown evaluation order");
	BN_REQUIRE(n_vars > 0 && n_vars < 40, "computing round evaluations requires at least a single variable");
	for (uint32_t e = 0; e < n_evs; e++) // (before any route looks at a composition)
		BN_REQUIRE(!(evs[e].composition && evs[e].composition->is_tower()) && !(evs[e].composition_at_infinity && evs[e].composition_at_infinity->is_tower()),
		           "a tower-typed expression is taken by bn_compute_composite alone");
	hal_request r{ctx, order, n_vars, d_tensor_query, query_vars, mls, n_mls, evs, n_evs, h_points, n_points, h_out, (uint64_t)1 << n_vars, (uint64_t)1 << (n_vars - 1)};
	r.acc = acc_scope{ctx};
	r.d_acc = ctx->d_result;
	// ---- the paths that take a whole request, wide ones included; they decline on input they do not know -- the checks come after
	routed res = route_coef(r);
	if (res.kind != routed::declined) return answered_by(r, BN_HALCNT_COEF, res.rc);
	const bool wide = is_wide(r);
	res = route_eq_set(r, wide);
	if (res.kind != routed::declined) return answered_by(r, BN_HALCNT_EQ_SET, res.rc);
	res = route_in_parts(r, wide);
	if (res.kind != routed::declined) return answered_by(r, BN_HALCNT_IN_PARTS, res.rc);
	// ---- one pass of the general code
	int rc = validate_evaluators(evs, n_evs, n_mls, h_points, n_points, /*one_pass=*/true, r.pts);
	if (rc) return rc;
	if (r.pts.total == 0) return BN_OK;
	rc = check_multilinears(r);
	if (rc) return rc;
	rc = plan_scratch(r);
	if (rc) return rc;
	rc = resolve_multilinears(r);
	if (rc) return rc;
	rc = r.acc.begin();
	if (rc) return rc;
	routed (*const routes[])(hal_request &) = {route_monomials, route_rows_batched, route_rows_per_point, route_interpreter};
	static_assert(BN_HALCNT_ROWS_BATCHED == BN_HALCNT_MONOMIALS + 1 && BN_HALCNT_ROWS_PER_POINT == BN_HALCNT_MONOMIALS + 2 &&
	                  BN_HALCNT_INTERPRETER == BN_HALCNT_MONOMIALS + 3,
	              "the counters of the four routes follow each other in the order the routes are tried");
	int route = BN_HALCNT_MONOMIALS;
	res = routes[0](r);
	while (res.kind == routed::declined && route < BN_HALCNT_INTERPRETER) res = routes[++route - BN_HALCNT_MONOMIALS](r);
	if (res.kind != routed::launched) return answered_by(r, route, res.rc);
	BN_HIP(hipMemcpyAsync(h_out, r.d_acc, r.pts.total * sizeof(f128), hipMemcpyDeviceToHost, ctx->stream));
	BN_HIP(hipStreamSynchronize(ctx->stream));
	return answered_by(r, route, r.acc.end());
}

int bn_hal_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	for (int i = 0; i < BN_HALCNT_N; i++) counters[i] = ctx->hal_calls[i];
	counters[BN_HALCNT_N_CU] = (uint64_t)ctx->n_cu;
	return BN_OK;
}

int bn_hal_fold_multilinear(bn_ctx *ctx, uint32_t order, uint32_t n_vars, const bn_hal_multilinear *ml, const bn_f128 *challenge,
                            const void *d_tensor_query, uint32_t query_vars, void *d_out, uint64_t out_cap, uint64_t *out_len)
{
	BN_REQUIRE(ctx && ml && challenge && out_len && (d_out || out_cap == 0), "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(order == BN_ORDER_LOW_TO_HIGH || order == BN_ORDER_HIGH_TO_LOW, "unknown evaluation order");
	BN_REQUIRE(n_vars > 0 && n_vars < 40, "folding requires at least a single variable");
	const uint64_t full = (uint64_t)1 << n_vars, half = full >> 1;
	if (ml->kind == BN_HAL_ML_TRANSPARENT) {
		// switchover (sumcheck_folding.rs:58-112, 164-216): partial evaluation at the query that already holds this
		// round's challenge
		BN_REQUIRE(query_vars > 0 && d_tensor_query, "tensor query missing while a multilinear is still transparent");
		BN_REQUIRE(out_cap >= half, "output buffer too small");
		bn_hal_multilinear t = *ml;
		int rc = materialise(ctx, order, n_vars - 1, t, d_tensor_query, query_vars, nullptr, d_out);
		if (rc) return rc;
		*out_len = half;
		return BN_OK;
	}
	BN_REQUIRE(ml->kind == BN_HAL_ML_FOLDED, "unknown multilinear kind");
	const uint64_t len = ml->len < full ? ml->len : full;
	const f128 z = to_f(challenge), sfx = to_f(&ml->suffix_eval);
	const uint64_t n_out = order == BN_ORDER_LOW_TO_HIGH ? (len + 1) / 2 : (len < half ? len : half);
	BN_REQUIRE(out_cap >= n_out, "output buffer too small");
	if (order == BN_ORDER_LOW_TO_HIGH && n_out) {
		const char *a = (const char *)ml->d_evals, *b = (const char *)d_out;
		BN_REQUIRE(b + n_out * 16 <= a || a + len * 16 <= b, "Low-to-High fold: output must not overlap the input");
	}
	prof_scope ps(ctx, BN_PROF_FOLD);
	if (order == BN_ORDER_HIGH_TO_LOW && len == full && d_out == ml->d_evals) {
		// the ComputeLayer shape: in-place fold of the two halves
		BN_HIP(bn::launch_extrapolate_line(ctx->stream, ctx->n_cu, d_out, (const char *)ml->d_evals + half * 16, half, z));
	} else {
		BN_HIP(bn::launch_hal_fold_lerp(ctx->stream, ctx->n_cu, ml->d_evals, len, sfx, order, half, z, d_out, n_out));
	}
	*out_len = n_out;
	return BN_OK;
}

} // extern "C"
