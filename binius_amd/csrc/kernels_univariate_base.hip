// binius_amd/csrc/kernels_univariate_base.hip -- the univariate round of the univariate-skip zerocheck for the wide arms of
// core/src/constraint_system/prove.rs:483-490 (4 => B16, 5 => B32, 6 => B64, 7 => B128): the domain and the Lagrange coefficients
// stay in B8, the univariatized columns and the composition live in FBase = T_base, the product with eq(x) in B128.
//
// With k skipped variables, index i = u + 2^k x (u < 2^k), omega_j the B8 element whose tower bits are j, W = 2^(base - 3) bytes:
//     R_c(omega_j) = sum_x eq(x) * C_c(Mhat_1(omega_j, x), ...),   Mhat_i(omega, x) = sum_u L_u(omega) M_i(u + 2^k x)
// for 2^k <= j < d_c 2^k.  In the tower basis the B8 scalar L_u(omega_j) acts on each of the W byte coordinates of M_i on its own.
//
// Form (the choice; kernels_univariate.hip is the B8 arm and is left alone):
//   * One wave per workgroup, one lane per point j; the grid is (tile of x, composition, 64-point chunk of j).  A value of a step is
//     NW = max(1, W / 4) words, so the step values of one workgroup are n_steps * NW * 256 bytes of (dynamic) LDS: 64 KiB for 64
//     steps over B128, 1 KiB for b32_mul's five steps.  With the 13.3 KiB of fixed tables that is at most 77.3 KiB -- two workgroups
//     per CU of 160 KiB in the worst case, a dozen and more for the compositions the gadgets have.
//   * Mhat by logarithms.  log L_u(omega_j) of the lane's point sits in LDS as [u][lane] bytes (L_u(omega_j) != 0 outside the
//     domain).  Per (column, x) the wave first turns the block's 2^k * Wc bytes (Wc = the column's own width) into logarithms in LDS
//     -- 512 for a zero byte, which lands in the zero half of the exp table --, then every lane reads them back as broadcasts (four
//     per 8-byte read at Wc >= 4) and takes ONE table look-up per (u, byte coordinate): exp[log L + log m].  A B1 column keeps the
//     parity-mask form of the B8 arm, a B8 column is the Wc = 1 case; both give a B8 value in the low byte.
//   * The composition's products are tower products in T_base by the bilinear walk of gf128.hpp (mul_walk<base>), POW by square and
//     multiply.  No bit-planes: eq(x) * v is one walk of the B128 element eq(x) over the 2^base bits of v per (x, lane), into one
//     128-bit accumulator per lane -- the 8 * 2^(base - 3) planes of the B8 arm's form would be 128 registers at B32 and 512 at B128.
//   * Extrapolation stays on the host (abi_univariate.cpp: barycentric Lagrange in B8, coordinate by coordinate), as for the B8 arm.
// The per-tile sums go to scratch; k_uskipb_reduce XORs them over the tiles in a fixed order (deterministic) and applies the
// batching power of each composition.
#include <hip/hip_runtime.h>

#include "internal.hpp"

namespace bn {

namespace {

constexpr uint32_t kLanes = kUskipBaseLanes;

template <int BASE>
struct base_traits {
	static constexpr uint32_t W = 1u << (BASE - 3);      // bytes of a value
	static constexpr uint32_t NW = W < 4 ? 1 : W / 4;    // words of a value
};

// a * b in T_BASE, both given as words (BASE <= 6: in .lo)
template <int BASE>
__device__ __forceinline__ f128 base_mul(f128 a, f128 b)
{
	if constexpr (BASE == 7)
		return mul_slow(a, b);
	else
		return f128{mul_walk<BASE>(f128{a.lo, 0}, b.lo).lo, 0};
}

// e * v, e in B128, v in T_BASE
template <int BASE>
__device__ __forceinline__ f128 eq_mul(f128 e, f128 v)
{
	if constexpr (BASE == 7)
		return mul_slow(e, v);
	else
		return mul_walk<BASE>(e, v.lo);
}

template <int NW>
__device__ __forceinline__ f128 load_val(const uint32_t *s_val, uint32_t step, uint32_t t)
{
	uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
	for (int i = 0; i < NW; i++) w[i] = s_val[(step * NW + i) * kLanes + t];
	return f128{(uint64_t)w[1] << 32 | w[0], (uint64_t)w[3] << 32 | w[2]};
}

template <int NW>
__device__ __forceinline__ void store_val(uint32_t *s_val, uint32_t step, uint32_t t, f128 v)
{
	const uint32_t w[4] = {(uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32)};
#pragma unroll
	for (int i = 0; i < NW; i++) s_val[(step * NW + i) * kLanes + t] = w[i];
}

__device__ __forceinline__ uint32_t parity128(uint4 w, uint4 m)
{
	return (__popc(w.x & m.x) ^ __popc(w.y & m.y) ^ __popc(w.z & m.z) ^ __popc(w.w & m.w)) & 1;
}

template <int BASE>
__global__ __launch_bounds__(kLanes) void k_uskipb_evals(uskip_args a)
{
	constexpr uint32_t NW = base_traits<BASE>::NW;
	__shared__ uint16_t s_lg[256];                     // log m, 512 for m = 0
	__shared__ uint8_t s_ex[768];                      // exp[i], 0 from 512 on
	__shared__ uint8_t s_lgl[128 * kLanes];            // [u][lane]: log L_u(omega_j)
	__shared__ __attribute__((aligned(16))) uint16_t s_lm[128 * 16]; // the block's logarithms, [u][byte coordinate]
	extern __shared__ uint32_t s_val[];                // [step][word][lane]
	const uint32_t c = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
	const uint32_t k = a.k, K = 1u << k; // k <= 7: some d_c >= 2 and d_c 2^k <= 256
	const uint32_t jt = blockIdx.z * kLanes + t, nj = a.n_j[c];
	if (blockIdx.z * kLanes >= nj) return; // (the whole wave: no barrier is missed)
	const bool active = jt < nj;
	const uint32_t j = active ? K + jt : K; // (an idle lane computes at omega_{2^k} and writes nothing)
	for (uint32_t i = t; i < 768; i += kLanes) {
		if (i < 256) s_lg[i] = i ? (uint16_t)a.logexp[i] : (uint16_t)512;
		s_ex[i] = i < 512 ? a.logexp[256 + i] : (uint8_t)0;
	}
	for (uint32_t u = 0; u < K; u++) s_lgl[u * kLanes + t] = a.lag[u * 256 + j]; // (the host passes the logarithms, transposed)
	__syncthreads();
	const uint32_t s0 = a.step_off[c], s1 = a.step_off[c + 1];
	f128 acc = f128_zero();
	const uint64_t n_x = (uint64_t)1 << a.n_x_log;
	const uint64_t x0 = (uint64_t)tile * a.x_per_tile;
	const uint64_t x1 = x0 + a.x_per_tile < n_x ? x0 + a.x_per_tile : n_x;
	for (uint64_t x = x0; x < x1; x++) {
		const uint4 e4 = a.eq[x];
		f128 v = f128_zero();
		for (uint32_t s = s0; s < s1; s++) {
			const bn_step st = a.steps[s];
			switch (st.kind) {
			case BN_STEP_VAR: {
				const uskip_col col = a.cols[st.a];
				const uint64_t off = x << k; // first value of the block
				uint32_t w[4] = {0, 0, 0, 0};
				if (col.level == 0) {
					const uint4 blk4 = ((const uint4 *)col.ptr)[off >> 7];
					const uint4 *m = a.masks + (size_t)j * 8;
					if (k == 7) {
#pragma unroll
						for (int b = 0; b < 8; b++) w[0] |= parity128(blk4, m[b]) << b;
					} else {
						const uint32_t sh = (uint32_t)(off & 127);
						const uint64_t word = sh < 64 ? ((uint64_t)blk4.y << 32 | blk4.x) : ((uint64_t)blk4.w << 32 | blk4.z);
						const uint64_t blk = (word >> (sh & 63)) & (k == 6 ? ~0ull : ((1ull << K) - 1));
#pragma unroll
						for (int b = 0; b < 8; b++) {
							const uint4 mb = m[b];
							w[0] |= (uint32_t)(__popcll(blk & ((uint64_t)mb.y << 32 | mb.x)) & 1) << b;
						}
					}
				} else {
					const uint32_t wc = 1u << (col.level - 3), nb = K * wc; // bytes of a value, of the block (nb <= 2048)
					const uint8_t *blk = (const uint8_t *)col.ptr + off * wc;
					__syncthreads(); // the last block's logarithms have been read
					for (uint32_t i = t; i < nb; i += kLanes) s_lm[i] = s_lg[blk[i]];
					__syncthreads();
					if (wc >= 4) {
#pragma unroll
						for (uint32_t q = 0; q < NW; q++) {
							uint32_t r = 0;
							if (4 * q < wc) { // (uniform: a narrower column leaves the upper coordinates 0)
								for (uint32_t u = 0; u < K; u++) {
									const uint32_t ll = s_lgl[u * kLanes + t];
									const uint2 lm = *(const uint2 *)&s_lm[u * wc + 4 * q];
									r ^= (uint32_t)s_ex[ll + (lm.x & 0xffff)] | (uint32_t)s_ex[ll + (lm.x >> 16)] << 8 |
									     (uint32_t)s_ex[ll + (lm.y & 0xffff)] << 16 | (uint32_t)s_ex[ll + (lm.y >> 16)] << 24;
								}
							}
							w[q] = r;
						}
					} else {
						uint32_t r = 0;
						for (uint32_t u = 0; u < K; u++) {
							const uint32_t ll = s_lgl[u * kLanes + t];
							r ^= (uint32_t)s_ex[ll + s_lm[u * wc]];
							if (wc == 2) r ^= (uint32_t)s_ex[ll + s_lm[u * wc + 1]] << 8;
						}
						w[0] = r;
					}
				}
				v = f128{(uint64_t)w[1] << 32 | w[0], (uint64_t)w[3] << 32 | w[2]};
				break;
			}
			case BN_STEP_CONST: v = f128{st.cst.lo, st.cst.hi}; break;
			case BN_STEP_ADD: v = load_val<NW>(s_val, st.a, t) ^ load_val<NW>(s_val, (uint32_t)st.b, t); break;
			case BN_STEP_MUL: v = base_mul<BASE>(load_val<NW>(s_val, st.a, t), load_val<NW>(s_val, (uint32_t)st.b, t)); break;
			default: { // BN_STEP_POW (kinds are validated on the host): square and multiply from the top bit of the exponent
				const f128 b = load_val<NW>(s_val, st.a, t);
				v = f128_one();
				for (int i = 63 - __clzll((long long)(st.b | 1)); i >= 0; i--) {
					v = base_mul<BASE>(v, v);
					if ((st.b >> i) & 1) v = base_mul<BASE>(v, b);
				}
				break;
			}
			}
			store_val<NW>(s_val, s - s0, t, v);
		}
		acc ^= eq_mul<BASE>(f128{(uint64_t)e4.y << 32 | e4.x, (uint64_t)e4.w << 32 | e4.z}, v);
	}
	if (active) ((f128 *)a.partial)[((size_t)c * a.n_tiles + tile) * a.th + jt] = acc;
}

// out[c][t] = scale[c] * XOR over tiles of partial[c][tile][t] (t < n_j[c]; 0 beyond); scale == nullptr: 1
__global__ void k_uskipb_reduce(const f128 *partial, uint32_t n_tiles, uint32_t th, uint32_t n_comps, const uint32_t *n_j, const f128 *scale, f128 *out)
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

template <int BASE>
hipError_t launch_one(hipStream_t s, const uskip_args &a, dim3 grid, uint32_t lds)
{
	// the static tables take 13.3 KiB: from 48 KiB of step values on, the launch needs the raised limit
	if (lds > 48 * 1024) {
		const hipError_t e = hipFuncSetAttribute((const void *)k_uskipb_evals<BASE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(k_uskipb_evals<BASE>, grid, dim3(kLanes), lds, s, a);
	return hipGetLastError();
}

} // namespace

uint32_t uskip_base_lds_bytes(uint32_t base_level, uint32_t max_steps)
{
	const uint32_t w = 1u << (base_level - 3);
	return max_steps * (w < 4 ? 1 : w / 4) * kLanes * 4;
}

hipError_t launch_uskip_evals_base(hipStream_t s, uint32_t base_level, const uskip_args &a, uint32_t max_steps, uint32_t n_comps, const f128 *scale, f128 *d_out)
{
	const dim3 grid(a.n_tiles, n_comps, a.th / kLanes);
	const uint32_t lds = uskip_base_lds_bytes(base_level, max_steps);
	hipError_t e;
	switch (base_level) {
	case 4: e = launch_one<4>(s, a, grid, lds); break;
	case 5: e = launch_one<5>(s, a, grid, lds); break;
	case 6: e = launch_one<6>(s, a, grid, lds); break;
	case 7: e = launch_one<7>(s, a, grid, lds); break;
	default: return hipErrorInvalidValue;
	}
	if (e != hipSuccess) return e;
	const uint64_t total = (uint64_t)n_comps * a.th;
	hipLaunchKernelGGL(k_uskipb_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const f128 *)a.partial, a.n_tiles, a.th, n_comps, a.n_j, scale, d_out);
	return hipGetLastError();
}

} // namespace bn
