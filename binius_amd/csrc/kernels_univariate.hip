// binius_amd/csrc/kernels_univariate.hip -- the univariate round of the univariate-skip zerocheck
// (crates/core/src/protocols/sumcheck/prove/univariate.rs:235-507, zerocheck_univariate_evals) over small-field columns.
//
// With k skipped variables, index i = u + 2^k x (u < 2^k), and omega_j the B8 element whose tower bits are j:
//     R_c(omega_j) = sum_x eq(x) * C_c(Mhat_1(omega_j, x), ..., Mhat_m(omega_j, x)),   Mhat_i(omega, x) = sum_u L_u(omega) M_i(u + 2^k x)
// for 2^k <= j < d_c 2^k.  Mhat lies in B8 and is GF(2)-linear in the block: for a B1 column bit b of Mhat_i(omega_j, x) is the parity
// of (block AND mask[j][b]), mask[j][b] = {u : bit b of L_u(omega_j)} -- one 2^k-bit block per (column, x), one 128-bit word at k = 7.
// For a B8 column it is sum_u L_u(omega_j) * M_i(u + 2^k x) in B8 (log / exp tables).
//
// Form: one workgroup per (tile of x, composition), one lane per point j.  Along the tile every lane reads the same block and the
// same eq(x) (uniform loads), evaluates the composition's steps in B8 (values in LDS, one byte per step and lane), and accumulates
// eq(x) * v as eight bit-planes: acc_b ^= eq(x) where bit b of v is set -- the GF(2)-linear form of the B8 x B128 product, whose
// basis factors 2^b are applied once at the end.  The per-tile sums go to scratch; k_uskip_reduce XORs them over the tiles (fixed
// order: the result is deterministic) and applies the batching power of each composition.
#include <hip/hip_runtime.h>

#include "internal.hpp"

namespace bn {

namespace {

__device__ __forceinline__ uint32_t b8_mul(const uint8_t *lg, const uint8_t *ex, uint32_t a, uint32_t b)
{
	if (!a || !b) return 0;
	return ex[(uint32_t)lg[a] + lg[b]]; // exp table of 512 entries: no reduction mod 255
}

__device__ __forceinline__ uint32_t b8_pow(const uint8_t *lg, const uint8_t *ex, uint32_t a, uint64_t e)
{
	if (e == 0) return 1;
	if (!a) return 0;
	return ex[(uint32_t)(((uint64_t)lg[a] * (e % 255)) % 255)];
}

__device__ __forceinline__ uint32_t parity128(uint4 w, uint4 m)
{
	return (__popc(w.x & m.x) ^ __popc(w.y & m.y) ^ __popc(w.z & m.z) ^ __popc(w.w & m.w)) & 1;
}

template <int TH>
__global__ __launch_bounds__(TH) void k_uskip_evals(uskip_args a)
{
	__shared__ uint8_t s_log[256];
	__shared__ uint8_t s_exp[512];
	__shared__ uint8_t s_val[kUskipMaxSteps][TH];
	for (uint32_t i = threadIdx.x; i < 768; i += TH) {
		if (i < 256)
			s_log[i] = a.logexp[i];
		else
			s_exp[i - 256] = a.logexp[i];
	}
	__syncthreads();
	const uint32_t c = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
	const uint32_t nj = a.n_j[c];
	if (t >= nj) return; // (no barrier below)
	// k <= 7 here: the host launches only when some d_c >= 2, and d_c 2^k <= 256 then bounds k -- so a B1 block is at most one
	// 128-bit word and the shift below never reaches 64
	const uint32_t k = a.k, j = (1u << k) + t;
	uint4 m[8];
#pragma unroll
	for (int b = 0; b < 8; b++) m[b] = a.masks[j * 8 + b];
	const uint8_t *lag = a.lag + (size_t)j * 256;
	const uint32_t s0 = a.step_off[c], s1 = a.step_off[c + 1];
	uint4 acc[8];
#pragma unroll
	for (int b = 0; b < 8; b++) acc[b] = make_uint4(0, 0, 0, 0);
	const uint64_t n_x = (uint64_t)1 << a.n_x_log;
	const uint64_t x0 = (uint64_t)tile * a.x_per_tile;
	const uint64_t x1 = x0 + a.x_per_tile < n_x ? x0 + a.x_per_tile : n_x;
	for (uint64_t x = x0; x < x1; x++) {
		const uint4 e = a.eq[x];
		uint32_t v = 0;
		for (uint32_t s = s0; s < s1; s++) {
			const bn_step st = a.steps[s];
			switch (st.kind) {
			case BN_STEP_VAR: {
				const uskip_col col = a.cols[st.a];
				const uint64_t off = x << k; // first value of the block
				v = 0;
				if (col.level == 0) {
					const uint4 w = ((const uint4 *)col.ptr)[off >> 7];
					if (k == 7) {
#pragma unroll
						for (int b = 0; b < 8; b++) v |= parity128(w, m[b]) << b;
					} else {
						const uint32_t sh = (uint32_t)(off & 127);
						const uint64_t word = sh < 64 ? ((uint64_t)w.y << 32 | w.x) : ((uint64_t)w.w << 32 | w.z);
						const uint64_t blk = (word >> (sh & 63)) & (k == 6 ? ~0ull : ((1ull << (1u << k)) - 1));
#pragma unroll
						for (int b = 0; b < 8; b++) v |= (uint32_t)(__popcll(blk & ((uint64_t)m[b].y << 32 | m[b].x)) & 1) << b;
					}
				} else {
					const uint8_t *blk = (const uint8_t *)col.ptr + off;
					for (uint32_t u = 0; u < (1u << k); u++) v ^= b8_mul(s_log, s_exp, blk[u], lag[u]);
				}
				break;
			}
			case BN_STEP_CONST: v = (uint32_t)(st.cst.lo & 0xff); break;
			case BN_STEP_ADD: v = (uint32_t)s_val[st.a][t] ^ s_val[st.b][t]; break;
			case BN_STEP_MUL: v = b8_mul(s_log, s_exp, s_val[st.a][t], s_val[st.b][t]); break;
			default: v = b8_pow(s_log, s_exp, s_val[st.a][t], st.b); break; // BN_STEP_POW (kinds are validated on the host)
			}
			s_val[s - s0][t] = (uint8_t)v;
		}
#pragma unroll
		for (int b = 0; b < 8; b++) {
			const uint32_t msk = 0u - ((v >> b) & 1);
			acc[b].x ^= e.x & msk;
			acc[b].y ^= e.y & msk;
			acc[b].z ^= e.z & msk;
			acc[b].w ^= e.w & msk;
		}
	}
	f128 r = f128_zero();
#pragma unroll
	for (int b = 0; b < 8; b++) r ^= mul_basis(f128{(uint64_t)acc[b].y << 32 | acc[b].x, (uint64_t)acc[b].w << 32 | acc[b].z}, (unsigned)b);
	((f128 *)a.partial)[((size_t)c * a.n_tiles + tile) * TH + t] = r;
}

// out[c][t] = scale[c] * XOR over tiles of partial[c][tile][t] (t < n_j[c]; 0 beyond); scale == nullptr: 1
__global__ void k_uskip_reduce(const f128 *partial, uint32_t n_tiles, uint32_t th, uint32_t n_comps, const uint32_t *n_j, const f128 *scale, f128 *out)
{
	const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (uint64_t)n_comps * th) return;
	const uint32_t c = (uint32_t)(idx / th), t = (uint32_t)(idx % th);
	f128 r = f128_zero();
	if (t < n_j[c]) {
		for (uint32_t tile = 0; tile < n_tiles; tile++) r ^= partial[((size_t)c * n_tiles + tile) * th + t];
		if (scale) r = mul_slow(r, scale[c]);
	}
	out[idx] = r;
}

} // namespace

hipError_t launch_uskip_evals(hipStream_t s, const uskip_args &a, uint32_t th, uint32_t n_comps, const f128 *scale, f128 *d_out)
{
	const dim3 grid(a.n_tiles, n_comps);
	if (th == 64)
		hipLaunchKernelGGL(k_uskip_evals<64>, grid, dim3(64), 0, s, a);
	else if (th == 128)
		hipLaunchKernelGGL(k_uskip_evals<128>, grid, dim3(128), 0, s, a);
	else
		hipLaunchKernelGGL(k_uskip_evals<256>, grid, dim3(256), 0, s, a);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	const uint64_t total = (uint64_t)n_comps * th;
	hipLaunchKernelGGL(k_uskip_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const f128 *)a.partial, a.n_tiles, th, n_comps, a.n_j, scale, d_out);
	return hipGetLastError();
}

} // namespace bn
