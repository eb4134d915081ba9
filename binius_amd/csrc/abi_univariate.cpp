// binius_amd/csrc/abi_univariate.cpp -- bn_zerocheck_univariate_evals: the univariate round of the univariate-skip zerocheck
// (crates/core/src/protocols/sumcheck/prove/univariate.rs:235-507) for the reference's `0..=3 => B8` arm
// (core/src/constraint_system/prove.rs:484): domain field B8, columns in B1 or B8, compositions over B8.  The host builds the
// Lagrange tables over the B8 points omega_0 .. omega_{2^k - 1} (omega_j = the element whose tower bits are j), the kernels of
// kernels_univariate.hip produce R_c(omega_j) for 2^k <= j < d_c 2^k, and the host extrapolates to the max domain
// (extrapolate_round_evals, univariate.rs:571-640) with barycentric Lagrange weights in B8.  Any method is bit-exact here: the
// polynomial of degree < d_c 2^k through those values and the 2^k zeros in front is unique.
//
// bn_zerocheck_univariate_evals_base is the same round for the wide arms (:485-488, 4 => B16 .. 7 => B128): the same host tables,
// validation and extrapolation -- the domain stays B8 --, with columns up to the base level, constants in the base field and the
// kernels of kernels_univariate_base.hip.  base_level 3 forwards to the entry point above.
#include <algorithm>

#include "abi_common.hpp"
#include "hostmul.hpp"

namespace {

// B8 in the tower basis: products, inverses, a log / exp pair for the kernels
struct b8_tables {
	uint8_t mul[256][256];
	uint8_t inv[256];
	uint8_t logexp[768]; // log[256] | exp[512], exp[i] = g^(i mod 255)
	b8_tables()
	{
		for (uint32_t a = 0; a < 256; a++)
			for (uint32_t b = 0; b < 256; b++) mul[a][b] = (uint8_t)(bn::mul_walk<3>(f128{a, 0}, b).lo & 0xff);
		inv[0] = 0;
		for (uint32_t a = 1; a < 256; a++)
			for (uint32_t b = 1; b < 256; b++)
				if (mul[a][b] == 1) {
					inv[a] = (uint8_t)b;
					break;
				}
		auto pw = [&](uint32_t x, uint32_t e) {
			uint32_t r = 1;
			while (e--) r = mul[r][x];
			return r;
		};
		uint32_t g = 2; // a generator: order 255 = 3 * 5 * 17
		while (pw(g, 85) == 1 || pw(g, 51) == 1 || pw(g, 15) == 1) g++;
		uint8_t *lg = logexp, *ex = logexp + 256;
		lg[0] = 0;
		uint32_t x = 1;
		for (uint32_t i = 0; i < 255; i++) {
			lg[x] = (uint8_t)i;
			x = mul[x][g];
		}
		for (uint32_t i = 0; i < 512; i++) ex[i] = (uint8_t)pw(g, i % 255);
	}
};

const b8_tables &b8()
{
	static const b8_tables t;
	return t;
}

// B8 scalar times a GF(2^128) element: in the tower basis the subfield acts on each of the 16 B8 coordinates
f128 mul_b8(f128 v, uint8_t s)
{
	const b8_tables &T = b8();
	f128 r{0, 0};
	for (int i = 0; i < 8; i++) {
		r.lo |= (uint64_t)T.mul[s][(v.lo >> (8 * i)) & 0xff] << (8 * i);
		r.hi |= (uint64_t)T.mul[s][(v.hi >> (8 * i)) & 0xff] << (8 * i);
	}
	return r;
}

// barycentric weights of the domain omega_0 .. omega_{n-1}: w_p = 1 / prod_{q != p} (omega_p - omega_q)
std::vector<uint8_t> bary_weights(uint32_t n)
{
	const b8_tables &T = b8();
	std::vector<uint8_t> w(n);
	for (uint32_t p = 0; p < n; p++) {
		uint32_t d = 1;
		for (uint32_t q = 0; q < n; q++)
			if (q != p) d = T.mul[d][p ^ q];
		w[p] = T.inv[d];
	}
	return w;
}

// ell_p(omega_j) of the domain omega_0 .. omega_{n-1} for a point j >= n outside it: w_p L(omega_j) / (omega_j - omega_p)
void lagrange_row(uint32_t n, const std::vector<uint8_t> &w, uint32_t j, uint8_t *out)
{
	const b8_tables &T = b8();
	uint32_t l = 1;
	for (uint32_t q = 0; q < n; q++) l = T.mul[l][j ^ q];
	for (uint32_t p = 0; p < n; p++) out[p] = T.mul[T.mul[w[p]][l]][T.inv[j ^ p]];
}

// r[t] = R(omega_{2^k + t}) for 2^k <= 2^k + t < d 2^k; zeros on omega_0 .. omega_{2^k - 1}: dst[j - 2^k] = P(omega_j), 2^k <= j < D
void extrapolate(uint32_t k, uint32_t d, uint32_t D, const f128 *r, f128 *dst)
{
	const uint32_t K = 1u << k, N = d << k;
	if (d < 2) return; // (P = 0)
	for (uint32_t j = K; j < N && j < D; j++) dst[j - K] = r[j - K];
	if (N >= D) return;
	const std::vector<uint8_t> w = bary_weights(N);
	std::vector<uint8_t> row(N);
	for (uint32_t j = N; j < D; j++) {
		lagrange_row(N, w, j, row.data());
		f128 acc{0, 0};
		for (uint32_t p = K; p < N; p++) acc ^= mul_b8(r[p - K], row[p]);
		dst[j - K] = acc;
	}
}

// is the constant an element of T_base (base 3 .. 7)?
bool const_in_base(const bn_f128 &c, uint32_t base) { return base >= 7 || (c.hi == 0 && (base == 6 || c.lo < ((uint64_t)1 << (1u << base)))); }

// the round over T_base: base 3 is the B8 arm (kernels_univariate.hip), 4 .. 7 the wide arms (kernels_univariate_base.hip)
int univariate_evals(bn_ctx *ctx, uint32_t base, uint32_t n_vars, uint32_t skip_rounds, const bn_hal_multilinear *mls, uint32_t n_mls, const bn_step *steps,
                     const uint32_t *step_offsets, const uint32_t *degrees, uint32_t n_comps, const void *d_eq, uint64_t eq_len, uint32_t max_domain_size,
                     const bn_f128 *h_batch_coeff, bn_f128 *h_out)
{
	BN_REQUIRE(ctx && h_out && (mls || n_mls == 0) && (n_comps == 0 || (steps && step_offsets && degrees)), "null argument");
	BN_ENTER(ctx);
	const uint32_t k = skip_rounds;
	BN_REQUIRE(k > 0, "skip_rounds must be at least 1");
	BN_REQUIRE(k <= n_vars, "too many skipped rounds (skip_rounds > n_vars)"); // Error::TooManySkippedRounds
	BN_REQUIRE(n_vars < 40, "n_vars out of range");
	BN_REQUIRE(k <= 8, "skip_rounds above the B8 domain");
	uint32_t d_max = 0;
	for (uint32_t c = 0; c < n_comps; c++) {
		BN_REQUIRE(degrees[c] >= 1, "composition of degree 0");
		BN_REQUIRE(((uint64_t)degrees[c] << k) <= 256, "d_c * 2^skip_rounds exceeds the B8 domain (256 points)");
		d_max = std::max(d_max, degrees[c]);
	}
	BN_REQUIRE(max_domain_size <= 256, "max_domain_size exceeds the B8 domain (256 points)");
	BN_REQUIRE(max_domain_size >= (1u << k) && max_domain_size >= (d_max << k), "Lagrange domain too small (max_domain_size < d_c * 2^skip_rounds)");
	const uint64_t n_vals = (uint64_t)1 << n_vars;
	for (uint32_t i = 0; i < n_mls; i++) {
		const bn_hal_multilinear &ml = mls[i];
		BN_REQUIRE(ml.kind == BN_HAL_ML_TRANSPARENT, "univariate round: columns are TRANSPARENT multilinears");
		if (base == 3)
			BN_REQUIRE(ml.tower_level == 0 || ml.tower_level == 3, "univariate round: column tower level must be 0 (B1) or 3 (B8)");
		else
			BN_REQUIRE(ml.tower_level == 0 || (ml.tower_level >= 3 && ml.tower_level <= base), "univariate round: column tower level must be 0 (B1) or 3 .. base_level");
		BN_REQUIRE(ml.n_vars_ml == n_vars, "univariate round: column n_vars_ml must equal n_vars");
		const uint64_t want = std::max<uint64_t>(1, n_vals >> (7 - ml.tower_level));
		BN_REQUIRE(ml.len == want && ml.d_evals, "univariate round: packed column length does not match n_vars");
	}
	BN_REQUIRE(n_comps == 0 || step_offsets[0] == 0, "step offsets must start at 0");
	for (uint32_t c = 0; c < n_comps; c++) {
		const uint32_t s0 = step_offsets[c], s1 = step_offsets[c + 1];
		BN_REQUIRE(s1 > s0 && s1 - s0 <= bn::kUskipMaxSteps, "composition with no steps or more than 64");
		for (uint32_t s = s0; s < s1; s++) {
			const bn_step &st = steps[s];
			const uint32_t i = s - s0;
			switch (st.kind) {
			case BN_STEP_VAR: BN_REQUIRE(st.a < n_mls, "composition uses more variables than there are columns"); break;
			case BN_STEP_CONST:
				if (base == 3)
					BN_REQUIRE(st.cst.hi == 0 && st.cst.lo < 256, "composition constant outside B8");
				else
					BN_REQUIRE(const_in_base(st.cst, base), "composition constant outside the base field");
				break;
			case BN_STEP_ADD:
			case BN_STEP_MUL: BN_REQUIRE(st.a < i && st.b < i, "composition step refers forward"); break;
			case BN_STEP_POW: BN_REQUIRE(st.a < i, "composition step refers forward"); break;
			default: return bn::fail(BN_ERR_INPUT_VALIDATION, "input validation: unknown composition step");
			}
		}
	}
	const uint32_t K = 1u << k, n_out = max_domain_size - K;
	const size_t out_count = h_batch_coeff ? n_out : (size_t)n_comps * n_out;
	std::fill(h_out, h_out + out_count, bn_f128{0, 0});
	const uint32_t nj_max = (d_max - 1) << k; // d_max >= 2 <=> some point to evaluate (then 2^k <= 128)
	if (n_comps == 0 || n_out == 0 || d_max < 2) return BN_OK;
	BN_REQUIRE(d_eq && eq_len == ((uint64_t)1 << (n_vars - k)), "eq table: 2^(n_vars - skip_rounds) elements");
	BN_FLUSH(ctx);

	// ---- host tables and the argument block, uploaded in one copy
	const b8_tables &T = b8();
	std::vector<uint8_t> lag(256 * 256, 0);
	std::vector<bn::f128> masks(256 * 8, bn::f128{0, 0});
	{
		const std::vector<uint8_t> w = bary_weights(K);
		for (uint32_t j = K; j < 256; j++) {
			lagrange_row(K, w, j, &lag[(size_t)j * 256]);
			for (uint32_t u = 0; u < K; u++)
				for (uint32_t b = 0; b < 8; b++)
					if ((lag[(size_t)j * 256 + u] >> b) & 1) {
						if (u < 64)
							masks[j * 8 + b].lo |= 1ull << u;
						else
							masks[j * 8 + b].hi |= 1ull << (u - 64);
					}
		}
	}
	// base 3: one workgroup of th lanes per (tile, composition); wide: one wave per (tile, composition, 64 points), th = the chunks' lanes
	if (base > 3) {
		// the wide kernel reads log L_u(omega_j) at u * 256 + j: the lanes of a wave (consecutive j) read consecutive bytes
		std::vector<uint8_t> lgl(256 * 256, 0);
		for (uint32_t j = K; j < 256; j++)
			for (uint32_t u = 0; u < K; u++) lgl[(size_t)u * 256 + j] = T.logexp[lag[(size_t)j * 256 + u]];
		lag.swap(lgl);
	}
	const uint32_t th = base > 3 ? (nj_max + bn::kUskipBaseLanes - 1) / bn::kUskipBaseLanes * bn::kUskipBaseLanes : nj_max <= 64 ? 64 : nj_max <= 128 ? 128 : 256;
	const uint32_t n_x_log = n_vars - k;
	const uint64_t n_x = (uint64_t)1 << n_x_log;
	const uint64_t wg_per_tile = base > 3 ? (uint64_t)n_comps * (th / bn::kUskipBaseLanes) : n_comps;
	uint64_t n_tiles = std::max<uint64_t>(1, std::min<uint64_t>(n_x, 2048 / wg_per_tile));
	const uint64_t x_per_tile = (n_x + n_tiles - 1) / n_tiles;
	n_tiles = (n_x + x_per_tile - 1) / x_per_tile;
	std::vector<bn::uskip_col> cols(std::max<uint32_t>(1, n_mls));
	for (uint32_t i = 0; i < n_mls; i++) cols[i] = bn::uskip_col{mls[i].d_evals, mls[i].tower_level, 0};
	const uint32_t n_steps = step_offsets[n_comps];
	std::vector<uint32_t> n_j(n_comps);
	for (uint32_t c = 0; c < n_comps; c++) n_j[c] = (degrees[c] - 1) << k;
	std::vector<bn::f128> scale;
	if (h_batch_coeff) {
		scale.resize(n_comps);
		bn::f128 p = bn::f128_one();
		for (uint32_t c = 0; c < n_comps; c++) {
			scale[c] = p;
			p = bn::mul_host(p, to_f(h_batch_coeff));
		}
	}
	call_upload up(ctx);
	const auto s_cols = up.reserve<bn::uskip_col>(cols.size());
	const auto s_steps = up.reserve<bn_step>(n_steps);
	const auto s_soff = up.reserve<uint32_t>(n_comps + 1);
	const auto s_nj = up.reserve<uint32_t>(n_comps);
	const auto s_masks = up.reserve<bn::f128>(masks.size());
	const auto s_lag = up.reserve<uint8_t>(lag.size());
	const auto s_logexp = up.reserve<uint8_t>(sizeof(T.logexp));
	const auto s_scale = up.reserve<bn::f128>(scale.size());
	up.device_only();
	const auto s_partial = up.reserve<bn::f128>((size_t)n_comps * n_tiles * th);
	const auto s_out = up.reserve<bn::f128>((size_t)n_comps * th);
	if (const int rc = up.alloc()) return rc;
	std::copy(cols.begin(), cols.end(), up.host(s_cols));
	std::copy(steps, steps + n_steps, up.host(s_steps));
	std::copy(step_offsets, step_offsets + n_comps + 1, up.host(s_soff));
	std::copy(n_j.begin(), n_j.end(), up.host(s_nj));
	std::copy(masks.begin(), masks.end(), up.host(s_masks));
	std::copy(lag.begin(), lag.end(), up.host(s_lag));
	std::copy(T.logexp, T.logexp + sizeof(T.logexp), up.host(s_logexp));
	std::copy(scale.begin(), scale.end(), up.host(s_scale));
	BN_HIP(up.send());
	bn::uskip_args a{};
	a.cols = up.dev(s_cols);
	a.steps = up.dev(s_steps);
	a.step_off = up.dev(s_soff);
	a.n_j = up.dev(s_nj);
	a.masks = (const uint4 *)up.dev(s_masks);
	a.lag = up.dev(s_lag);
	a.logexp = up.dev(s_logexp);
	a.eq = (const uint4 *)d_eq;
	a.partial = up.dev(s_partial);
	a.k = k;
	a.n_x_log = n_x_log;
	a.n_tiles = (uint32_t)n_tiles;
	a.th = th;
	a.x_per_tile = x_per_tile;
	{
		prof_scope ps(ctx, BN_PROF_ROUND_EVAL);
		if (base > 3) {
			uint32_t max_steps = 0;
			for (uint32_t c = 0; c < n_comps; c++) max_steps = std::max(max_steps, step_offsets[c + 1] - step_offsets[c]);
			BN_HIP(bn::launch_uskip_evals_base(ctx->stream, base, a, max_steps, n_comps, scale.empty() ? nullptr : up.dev(s_scale), up.dev(s_out)));
		} else {
			BN_HIP(bn::launch_uskip_evals(ctx->stream, a, th, n_comps, scale.empty() ? nullptr : up.dev(s_scale), up.dev(s_out)));
		}
	}
	std::vector<bn::f128> r((size_t)n_comps * th);
	BN_HIP(hipMemcpyAsync(r.data(), up.dev(s_out), r.size() * sizeof(bn::f128), hipMemcpyDeviceToHost, ctx->stream));
	BN_HIP(hipStreamSynchronize(ctx->stream));

	// ---- extrapolation to the max domain: per composition, or per degree class of the batched sum (extrapolation is linear)
	std::vector<bn::f128> dst(n_out);
	if (!h_batch_coeff) {
		for (uint32_t c = 0; c < n_comps; c++) {
			std::fill(dst.begin(), dst.end(), bn::f128_zero());
			extrapolate(k, degrees[c], max_domain_size, &r[(size_t)c * th], dst.data());
			for (uint32_t i = 0; i < n_out; i++) h_out[(size_t)c * n_out + i] = bn_f128{dst[i].lo, dst[i].hi};
		}
		return BN_OK;
	}
	std::vector<bn::f128> total(n_out, bn::f128_zero()), cls(th);
	for (uint32_t d = 2; d <= d_max; d++) {
		bool any = false;
		std::fill(cls.begin(), cls.end(), bn::f128_zero());
		for (uint32_t c = 0; c < n_comps; c++)
			if (degrees[c] == d) {
				any = true;
				for (uint32_t t = 0; t < th; t++) cls[t] ^= r[(size_t)c * th + t];
			}
		if (!any) continue;
		std::fill(dst.begin(), dst.end(), bn::f128_zero());
		extrapolate(k, d, max_domain_size, cls.data(), dst.data());
		for (uint32_t i = 0; i < n_out; i++) total[i] ^= dst[i];
	}
	for (uint32_t i = 0; i < n_out; i++) h_out[i] = bn_f128{total[i].lo, total[i].hi};
	return BN_OK;
}

} // namespace

extern "C" {

int bn_zerocheck_univariate_evals(bn_ctx *ctx, uint32_t n_vars, uint32_t skip_rounds, const bn_hal_multilinear *mls, uint32_t n_mls,
                                  const bn_step *steps, const uint32_t *step_offsets, const uint32_t *degrees, uint32_t n_comps, const void *d_eq,
                                  uint64_t eq_len, uint32_t max_domain_size, const bn_f128 *h_batch_coeff, bn_f128 *h_out)
{
	return univariate_evals(ctx, 3, n_vars, skip_rounds, mls, n_mls, steps, step_offsets, degrees, n_comps, d_eq, eq_len, max_domain_size, h_batch_coeff, h_out);
}

int bn_zerocheck_univariate_evals_base(bn_ctx *ctx, uint32_t base_level, uint32_t n_vars, uint32_t skip_rounds, const bn_hal_multilinear *mls, uint32_t n_mls,
                                       const bn_step *steps, const uint32_t *step_offsets, const uint32_t *degrees, uint32_t n_comps, const void *d_eq,
                                       uint64_t eq_len, uint32_t max_domain_size, const bn_f128 *h_batch_coeff, bn_f128 *h_out)
{
	BN_REQUIRE(ctx, "null argument");
	BN_REQUIRE(base_level >= 3 && base_level <= 7, "univariate round: base_level must be 3 (B8) .. 7 (B128)");
	if (base_level == 3) // constructor.create::<B8>(): the existing entry point, unchanged
		return bn_zerocheck_univariate_evals(ctx, n_vars, skip_rounds, mls, n_mls, steps, step_offsets, degrees, n_comps, d_eq, eq_len, max_domain_size, h_batch_coeff, h_out);
	return univariate_evals(ctx, base_level, n_vars, skip_rounds, mls, n_mls, steps, step_offsets, degrees, n_comps, d_eq, eq_len, max_domain_size, h_batch_coeff, h_out);
}

} // extern "C"
