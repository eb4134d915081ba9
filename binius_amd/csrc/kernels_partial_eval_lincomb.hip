// binius_amd/csrc/kernels_partial_eval_lincomb.hip -- the projection kernels_partial_eval.hip makes of a column, made of a LINEAR
// COMBINATION of columns that is never materialised (try_build_partial_eval, core/src/protocols/evalcheck/subclaims.rs:305-346: the
// inner column of a shifted or packed claim is itself a LinearCombination -- keccak's c[x], the sum of five state columns):
//   out_j[i] = offset_j + sum_t coeff_t * sum_q vec[q] * M_t[q * 2^b + i],   0 <= i < 2^b.
// The projection is linear, so terms of a job with equal (tower level, coefficient) -- a CLASS -- are XOR-ed as packed words when they
// are loaded and go through ONE row loop: the lane-mask loop of a bit column (pe_rows.hpp pe_block) at level 0, the subfield product
// at levels >= 3.  The row loop is where the time goes (VALU issue, not bytes), so five coefficient-ONE bit columns cost one loop.
//
// A unit (one workgroup) is a chunk of 2^log_ch indices q of one job: it stages its chunk of `vec` in LDS once and walks every class
// of the job from it.  The sums of a class are combined over the workgroup's threads in LDS, multiplied by the class's coefficient
// (once per workgroup and output; not at all for ONE), and XOR-ed into the workgroup's own 2^b sums in LDS; those go out at the end
// with 64-bit XOR atomics -- one pair per output and workgroup whatever the number of classes -- into outputs that k_pel_init
// filled with the job's offset.  Jobs with more than 2^kPeMaxLogOut outputs run one thread per output in a launch of their own.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "ctable.hpp"
#include "gf128.hpp"
#include "internal.hpp"
#include "pe_rows.hpp"

namespace bn {

namespace {

__device__ __noinline__ uint4 pel_scale(uint4 v, f128 coeff) { return to_u4(mul_slow(to_f128(v), coeff)); }

// XOR over the threads t' = o, o + P, o + 2P, .. of the workgroup's values, times the class's coefficient, into tot[o] (o < P; P a
// power of two <= 256)
template <bool BITS_ONE>
__device__ __forceinline__ void pel_emit(uint4 acc, uint4 *red, uint4 *tot, uint32_t P, f128 coeff, uint32_t one)
{
	__syncthreads(); // (the readers of the previous round are done)
	red[threadIdx.x] = acc;
	__syncthreads();
	if (threadIdx.x < P) {
		uint4 v{0, 0, 0, 0};
		for (uint32_t s = threadIdx.x; s < 256; s += P) v = xor4(v, red[s]);
		if constexpr (!BITS_ONE)
			if (!one) v = pel_scale(v, coeff);
		tot[threadIdx.x] = xor4(tot[threadIdx.x], v);
	}
}

// level 0: rows [j0, j0 + ch) of the XOR of the class's bit columns, 2^b outputs
template <bool BITS_ONE>
__device__ __forceinline__ void pel_bits(const uint64_t *const *__restrict__ cols, uint32_t n_cols, uint4 *tot, uint32_t b, uint64_t j0, uint32_t ch, const uint4 *lvec,
                                         uint4 *red, f128 coeff, uint32_t one)
{
	const uint32_t lane = threadIdx.x & 63, wave = uni32(threadIdx.x >> 6);
	const uint32_t T = b > 6 ? 1u << (b - 6) : 1u; // words per row
	const uint32_t sh = b < 6 ? 6 - b : 0;         // log2 of the rows per word
	const uint32_t S = ch >> sh;                   // steps of the chunk: rows (b >= 6) or words (b < 6); ch >= 2^sh (host)
	const uint64_t g0 = b >= 6 ? j0 << (b - 6) : j0 >> sh;
	const uint32_t sub = lane >> b;                // the lane's row inside a word (b < 6), else 0
	for (uint32_t t = 0; t < T; t++) {
		uint4 acc{0, 0, 0, 0};
		for (uint32_t s0 = wave * 64; s0 < S; s0 += 256) {
			const uint32_t s = s0 + lane;
			uint64_t w = 0;
			if (s < S) {
				// four columns a round, their loads in flight together (a loop over single columns waits for every word before it
				// reads the next pointer); a round past the end reads the last column again and drops the word
				const uint64_t at = g0 + (uint64_t)s * T + t;
				for (uint32_t c = 0; c < n_cols; c += 4) {
					const uint64_t *p[4]; // (all four pointers first: a load through one counts on the counter the next pointer waits for)
					uint64_t a[4];
#pragma unroll
					for (uint32_t k = 0; k < 4; k++) p[k] = (const uint64_t *)uni64((uint64_t)cols[c + k < n_cols ? c + k : n_cols - 1]);
					__builtin_amdgcn_sched_barrier(0);
#pragma unroll
					for (uint32_t k = 0; k < 4; k++) a[k] = p[k][at];
#pragma unroll
					for (uint32_t k = 0; k < 4; k++) w ^= c + k < n_cols ? a[k] : 0;
				}
			}
			const uint32_t w_lo = (uint32_t)w, w_hi = (uint32_t)(w >> 32);
			if (sh == 0)
				pe_block<false>(acc, w_lo, w_hi, lvec + s0, 0);
			else
				pe_block<true>(acc, w_lo, w_hi, lvec, ((s0 << sh) + sub) | (sh << 16));
		}
		pel_emit<BITS_ONE>(acc, red, tot + (uint64_t)t * 64, b < 6 ? 1u << b : 64u, coeff, one);
	}
}

// value idx of the XOR of the class's columns packed at tower level IOTA >= 3 (in .lo below level 7)
template <int IOTA>
__device__ __forceinline__ f128 pel_value(const uint64_t *const *__restrict__ cols, uint32_t n_cols, uint64_t idx)
{
	f128 v = f128_zero();
	if constexpr (IOTA == 7) {
		for (uint32_t c = 0; c < n_cols; c++) v ^= f128{cols[c][2 * idx], cols[c][2 * idx + 1]};
	} else if constexpr (IOTA == 6) {
		for (uint32_t c = 0; c < n_cols; c++) v.lo ^= cols[c][idx];
	} else {
		constexpr unsigned W = 1u << IOTA, PER = 64 / W;
		for (uint32_t c = 0; c < n_cols; c++) v.lo ^= cols[c][idx / PER];
		v.lo = (v.lo >> ((idx % PER) * W)) & ((1ull << W) - 1);
	}
	return v;
}
template <int IOTA>
__device__ __forceinline__ f128 pel_mul(f128 x, f128 v)
{
	if constexpr (IOTA == 7)
		return mul_slow(x, v);
	else
		return mul_walk<IOTA>(x, v.lo);
}

// levels >= 3: thread (i, slice) sums its slice of the rows [j0, j0 + ch)
template <int IOTA>
__device__ __noinline__ void pel_field(const uint64_t *const *__restrict__ cols, uint32_t n_cols, uint4 *tot, uint32_t b, uint64_t j0, uint32_t ch, const uint4 *lvec,
                                       uint4 *red, f128 coeff, uint32_t one)
{
	const uint32_t out_len = 1u << b, P = out_len < 256 ? out_len : 256u;
	const uint32_t slice = threadIdx.x / P, n_slices = 256 / P;
	for (uint32_t t = 0; t < out_len / P; t++) {
		const uint32_t i = t * P + (threadIdx.x & (P - 1));
		f128 acc = f128_zero();
		for (uint32_t j = slice; j < ch; j += n_slices) acc ^= pel_mul<IOTA>(to_f128(lvec[j]), pel_value<IOTA>(cols, n_cols, ((j0 + j) << b) + i));
		pel_emit<false>(to_u4(acc), red, tot + (uint64_t)t * P, P, coeff, one);
	}
}

} // namespace

__global__ __launch_bounds__(256) void k_pel_init(const pel_job *__restrict__ jobs, uint32_t n_jobs)
{
	if (blockIdx.x >= n_jobs) return;
	const pel_job &j = jobs[blockIdx.x];
	uint4 *o = reinterpret_cast<uint4 *>(j.out);
	const uint4 v = to_u4(j.offset);
	const uint32_t out_len = 1u << j.b;
	for (uint32_t i = threadIdx.x; i < out_len; i += 256) o[i] = v;
}

// BITS_ONE: every class of the launch is at level 0 with coefficient ONE.  The general instantiation carries the register allocation
// of mul_walk<6> into the bit path too (256 VGPRs, 40 AGPRs and scratch: one wave per SIMD); this one is the bit path alone (as
// k_partial_eval<true>).
template <bool BITS_ONE>
__global__ __launch_bounds__(256, BITS_ONE ? 4 : 1) void k_pel(const pel_job *__restrict__ jobs, uint32_t n_jobs, const pel_class *__restrict__ classes,
                                                             const uint64_t *const *__restrict__ cols, const uint4 *__restrict__ vec)
{
	__shared__ uint4 lvec[1u << kPeLogVecChunk];
	__shared__ uint4 red[256];
	extern __shared__ uint4 tot[]; // the workgroup's sums over all classes: 2^b of the launch's widest job
	if (n_jobs == 0) return;
	const pel_job &g = jobs[find_job(jobs, n_jobs, blockIdx.x)];
	const uint32_t first = uni32(g.first_class), count = uni32(g.n_classes), b = uni32(g.b), log_ch = uni32(g.log_ch);
	const uint32_t ch = 1u << log_ch, out_len = 1u << b;
	const uint64_t j0 = (uint64_t)(blockIdx.x - uni32(g.start)) << log_ch;
	uint64_t *out = (uint64_t *)uni64((uint64_t)g.out);
	for (uint32_t e = threadIdx.x; e < ch; e += 256) lvec[e] = vec[j0 + e];
	for (uint32_t i = threadIdx.x; i < out_len; i += 256) tot[i] = uint4{0, 0, 0, 0};
	for (uint32_t c = 0; c < count; c++) {
		const pel_class &k = classes[first + c];
		const uint64_t *const *kc = cols + uni32(k.first_col);
		const uint32_t n_cols = uni32(k.n_cols), one = uni32(k.one);
		const f128 coeff{uni64(k.coeff.lo), uni64(k.coeff.hi)};
		__syncthreads();
		if constexpr (BITS_ONE) {
			pel_bits<true>(kc, n_cols, tot, b, j0, ch, lvec, red, coeff, one);
		} else {
			switch (uni32(k.level)) {
			case 0: pel_bits<false>(kc, n_cols, tot, b, j0, ch, lvec, red, coeff, one); break;
			case 3: pel_field<3>(kc, n_cols, tot, b, j0, ch, lvec, red, coeff, one); break;
			case 4: pel_field<4>(kc, n_cols, tot, b, j0, ch, lvec, red, coeff, one); break;
			case 5: pel_field<5>(kc, n_cols, tot, b, j0, ch, lvec, red, coeff, one); break;
			case 6: pel_field<6>(kc, n_cols, tot, b, j0, ch, lvec, red, coeff, one); break;
			default: pel_field<7>(kc, n_cols, tot, b, j0, ch, lvec, red, coeff, one); break;
			}
		}
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < out_len; i += 256) {
		const uint4 v = tot[i];
		const uint64_t lo = (uint64_t)v.x | ((uint64_t)v.y << 32), hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
		unsigned long long *o = reinterpret_cast<unsigned long long *>(out) + 2 * (uint64_t)i;
		if (lo) atomicXor(o, (unsigned long long)lo);
		if (hi) atomicXor(o + 1, (unsigned long long)hi);
	}
}

// more than 2^kPeMaxLogOut outputs: thread = one output, written once (offset included; nothing is cleared for these jobs)
__global__ __launch_bounds__(256) void k_pel_wide(const pel_job *__restrict__ jobs, uint32_t n_jobs, const pel_class *__restrict__ classes,
                                                  const uint64_t *const *__restrict__ cols, const uint4 *__restrict__ vec, uint32_t q)
{
	const pel_job &g = jobs[find_job(jobs, n_jobs, blockIdx.x)];
	const uint32_t b = g.b;
	const uint64_t i = ((uint64_t)(blockIdx.x - g.start) << 8) + threadIdx.x; // (2^b is a multiple of 256)
	f128 res = g.offset;
	for (uint32_t c = 0; c < g.n_classes; c++) {
		const pel_class &k = classes[g.first_class + c];
		const uint64_t *const *kc = cols + k.first_col;
		f128 part = f128_zero();
		for (uint64_t j = 0; j < ((uint64_t)1 << q); j++) {
			const uint64_t idx = (j << b) + i;
			const f128 x = to_f128(vec[j]);
			switch (k.level) {
			case 0: {
				uint64_t w = 0;
				for (uint32_t t = 0; t < k.n_cols; t++) w ^= kc[t][idx >> 6];
				part ^= mul_walk<0>(x, w >> (idx & 63));
				break;
			}
			case 3: part ^= pel_mul<3>(x, pel_value<3>(kc, k.n_cols, idx)); break;
			case 4: part ^= pel_mul<4>(x, pel_value<4>(kc, k.n_cols, idx)); break;
			case 5: part ^= pel_mul<5>(x, pel_value<5>(kc, k.n_cols, idx)); break;
			case 6: part ^= pel_mul<6>(x, pel_value<6>(kc, k.n_cols, idx)); break;
			default: part ^= pel_mul<7>(x, pel_value<7>(kc, k.n_cols, idx)); break;
			}
		}
		res ^= k.one ? part : mul_slow(part, k.coeff);
	}
	reinterpret_cast<uint4 *>(g.out)[i] = to_u4(res);
}

hipError_t launch_partial_eval_lincomb(hipStream_t s, const pel_job *d_init, uint32_t n_init, const pel_job *d_jobs, uint32_t n_jobs, const pel_class *d_classes,
                                       const uint64_t *const *d_cols, const void *vec, uint32_t total_units, uint32_t lds_out, bool bits_one)
{
	if (n_init == 0) return hipSuccess; // (only wide jobs: nothing to clear, no unit to run)
	hipLaunchKernelGGL(k_pel_init, dim3(n_init), dim3(256), 0, s, d_init, n_init);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	const dim3 grid(n_jobs ? total_units : 1);
	const size_t lds = sizeof(uint4) * (lds_out ? lds_out : 1);
	if (bits_one)
		hipLaunchKernelGGL(k_pel<true>, grid, dim3(256), lds, s, d_jobs, n_jobs, d_classes, d_cols, (const uint4 *)vec);
	else
		hipLaunchKernelGGL(k_pel<false>, grid, dim3(256), lds, s, d_jobs, n_jobs, d_classes, d_cols, (const uint4 *)vec);
	return hipGetLastError();
}

hipError_t launch_partial_eval_lincomb_wide(hipStream_t s, const pel_job *d_jobs, uint32_t n_jobs, const pel_class *d_classes, const uint64_t *const *d_cols,
                                            const void *vec, uint32_t q, uint32_t total_units)
{
	if (n_jobs == 0 || total_units == 0) return hipSuccess;
	hipLaunchKernelGGL(k_pel_wide, dim3(total_units), dim3(256), 0, s, d_jobs, n_jobs, d_classes, d_cols, (const uint4 *)vec, q);
	return hipGetLastError();
}

} // namespace bn
