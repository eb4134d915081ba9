// binius_amd/csrc/kernels_partial_eval.hip -- a batch of columns evaluated at the high coordinates of one point: what evalcheck
// does to the inner column of every shifted or packed virtual column before its sumchecks start (collect_projected_mles,
// core/src/protocols/evalcheck/subclaims.rs:356-439: evaluate_partial_high, math/src/multilinear_extension.rs:253-300):
//   out_c[i] = sum_j vec[j] * M_c[j * 2^b + i],   0 <= i < 2^b,  vec = the tensor expansion of the high coordinates,
// the same sum bn_fold_left computes for one column, for 2^b <= 1024.  There the reduction index j is the long one (2^16 rows
// of 64 bits for a B1 column of 2^22 bits at b = 6) and the outputs are few, so the work is split over j: a unit (one workgroup)
// is a chunk of 2^log_ch indices j of a group of columns of one class (tower level, b).  The chunk of `vec` is staged in LDS
// once and serves every column of the group; partial sums are XOR-combined (exact, order-free) with 64-bit atomics into outputs
// that k_pe_zero cleared.  Two launches per call whatever the number of columns, their levels and sizes; units are found in the
// group table by bisection (as in kernels_prodtree.hip).
//
// Level 0 (bits): a 64-bit word of the column is a lane mask.  b >= 6: row j is 2^(b-6) words, lane l owns out[64 t + l] and a
// step is "acc ^= vec[j] under the mask" -- the word goes to a scalar register pair and becomes the execution mask of four
// XORs of a value every lane reads from the same LDS address.  b < 6: a word holds 2^(6-b) rows, lane l reads
// vec[row of l] and the lanes with equal l mod 2^b are combined at the end.  Each lane loads one word of 64 consecutive
// steps (a coalesced 512-byte request for b <= 6), the words are then broadcast one by one.
// Levels >= 3: threads over (i, a slice of j) with the generic subfield product (gf128.hpp mul_walk), as k_fold does it, the
// slices combined at the end.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "ctable.hpp"
#include "gf128.hpp"
#include "internal.hpp"
#include "pe_rows.hpp"

namespace bn {

namespace {

// XOR over the threads t' = o, o + P, o + 2P, .. of the workgroup's values, into out[o] (o < P; P a power of two <= 256)
__device__ __forceinline__ void pe_emit(uint4 acc, uint4 *red, uint64_t *out, uint32_t P)
{
	__syncthreads(); // (the readers of the previous round are done)
	red[threadIdx.x] = acc;
	__syncthreads();
	if (threadIdx.x < P) {
		uint4 v{0, 0, 0, 0};
		for (uint32_t s = threadIdx.x; s < 256; s += P) v = xor4(v, red[s]);
		const uint64_t lo = (uint64_t)v.x | ((uint64_t)v.y << 32), hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
		unsigned long long *o = reinterpret_cast<unsigned long long *>(out) + 2 * threadIdx.x;
		if (lo) atomicXor(o, (unsigned long long)lo);
		if (hi) atomicXor(o + 1, (unsigned long long)hi);
	}
}

// level 0: rows [j0, j0 + ch) of a bit column with 2^b outputs
__device__ __forceinline__ void pe_bits(const uint64_t *__restrict__ evals, uint64_t *out, uint32_t b, uint64_t j0, uint32_t ch, const uint4 *lvec, uint4 *red)
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
			const uint64_t w = s < S ? evals[g0 + (uint64_t)s * T + t] : 0;
			const uint32_t w_lo = (uint32_t)w, w_hi = (uint32_t)(w >> 32);
			if (sh == 0)
				pe_block<false>(acc, w_lo, w_hi, lvec + s0, 0);
			else
				pe_block<true>(acc, w_lo, w_hi, lvec, ((s0 << sh) + sub) | (sh << 16));
		}
		pe_emit(acc, red, out + 2 * (uint64_t)t * 64, b < 6 ? 1u << b : 64u);
	}
}

// levels >= 3: thread (i, slice) sums its slice of the rows [j0, j0 + ch)
template <int IOTA>
__device__ __noinline__ void pe_field(const uint64_t *__restrict__ evals, uint64_t *out, uint32_t b, uint64_t j0, uint32_t ch, const uint4 *lvec, uint4 *red)
{
	const uint32_t out_len = 1u << b, P = out_len < 256 ? out_len : 256u;
	const uint32_t slice = threadIdx.x / P, n_slices = 256 / P;
	for (uint32_t t = 0; t < out_len / P; t++) {
		const uint32_t i = t * P + (threadIdx.x & (P - 1));
		f128 acc = f128_zero();
		for (uint32_t j = slice; j < ch; j += n_slices) acc ^= pe_mul<IOTA>(to_f128(lvec[j]), evals, ((j0 + j) << b) + i);
		pe_emit(to_u4(acc), red, out + 2 * (uint64_t)t * P, P);
	}
}

} // namespace

__global__ __launch_bounds__(256) void k_pe_zero(const pe_col *__restrict__ cols, pe_col one_col)
{
	const pe_col c = cols ? cols[blockIdx.x] : one_col;
	uint4 *o = reinterpret_cast<uint4 *>(c.out);
	for (uint32_t i = threadIdx.x; i < c.out_len; i += 256) o[i] = uint4{0, 0, 0, 0};
}

// BITS_ONLY: every group of the launch is at level 0.  The general instantiation carries the register allocation of mul_walk<6>
// (256 VGPRs, scratch) into the bit path too; this one is the bit path alone.
template <bool BITS_ONLY>
__global__ __launch_bounds__(256, BITS_ONLY ? 4 : 2) void k_partial_eval(const pe_group *__restrict__ groups, uint32_t n_groups, const pe_col *__restrict__ cols, pe_group one_group,
                                                      pe_col one_col, const uint4 *__restrict__ vec)
{
	__shared__ uint4 lvec[1u << kPeLogVecChunk];
	__shared__ uint4 red[256];
	pe_group g = one_group;
	if (groups) g = groups[find_job(groups, n_groups, blockIdx.x)];
	const uint32_t first = uni32(g.first), count = uni32(g.count), level = uni32(g.level), b = uni32(g.b), log_ch = uni32(g.log_ch);
	const uint32_t ch = 1u << log_ch;
	const uint64_t j0 = (uint64_t)(blockIdx.x - uni32(g.start)) << log_ch;
	for (uint32_t e = threadIdx.x; e < ch; e += 256) lvec[e] = vec[j0 + e];
	for (uint32_t c = 0; c < count; c++) {
		const uint64_t *evals = (const uint64_t *)uni64((uint64_t)(cols ? cols[first + c].evals : one_col.evals));
		uint64_t *out = (uint64_t *)uni64((uint64_t)(cols ? cols[first + c].out : one_col.out));
		__syncthreads();
		if constexpr (BITS_ONLY) {
			pe_bits(evals, out, b, j0, ch, lvec, red);
		} else {
			switch (level) {
			case 0: pe_bits(evals, out, b, j0, ch, lvec, red); break;
			case 3: pe_field<3>(evals, out, b, j0, ch, lvec, red); break;
			case 4: pe_field<4>(evals, out, b, j0, ch, lvec, red); break;
			case 5: pe_field<5>(evals, out, b, j0, ch, lvec, red); break;
			case 6: pe_field<6>(evals, out, b, j0, ch, lvec, red); break;
			default: pe_field<7>(evals, out, b, j0, ch, lvec, red); break;
			}
		}
	}
}

hipError_t launch_partial_eval(hipStream_t s, const pe_group *d_groups, uint32_t n_groups, const pe_col *d_cols, uint32_t n_cols, pe_group one_group,
                               pe_col one_col, const void *vec, uint32_t total_units, bool bits_only)
{
	if (n_cols == 0 || total_units == 0) return hipSuccess;
	hipLaunchKernelGGL(k_pe_zero, dim3(n_cols), dim3(256), 0, s, d_cols, one_col);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	if (bits_only)
		hipLaunchKernelGGL(k_partial_eval<true>, dim3(total_units), dim3(256), 0, s, d_groups, n_groups, d_cols, one_group, one_col, (const uint4 *)vec);
	else
		hipLaunchKernelGGL(k_partial_eval<false>, dim3(total_units), dim3(256), 0, s, d_groups, n_groups, d_cols, one_group, one_col, (const uint4 *)vec);
	return hipGetLastError();
}

} // namespace bn
