// binius_amd/csrc/kernels_mle_eval.hip -- a batch of columns evaluated at their whole claim points: the first step of every
// EvalcheckProver::prove call (core/src/protocols/evalcheck/prove.rs:191-275, make_new_eval_claim :812-879), which splits the point
// into a prefix and a suffix, takes evaluate_partial_high of the column at the suffix and evaluates the result at the prefix
// (math/src/multilinear_extension.rs evaluate / evaluate_partial_high):
//   eval = sum_l lo[l] * (sum_h hi[h] * col[h * 2^b + l]),   lo / hi = the tensor expansions of the first b / the other q coordinates.
// The inner sum is what kernels_partial_eval.hip computes per output index; here the 2^b partial sums never leave the workgroup.
// A unit (one workgroup) is a chunk of 2^log_ch rows h of a group of jobs of one class (point, tower level).  It walks its chunk in
// stages of up to 2^kPeLogVecChunk rows: the stage of `hi` goes to LDS once and serves every job of the group; the per-index partial
// sums of a job are accumulated in LDS (accs, 2^b entries per job) with LDS XOR atomics, so the waves need no barrier between jobs.
// The epilogue multiplies every accumulator by its `lo` entry -- once per unit, job and index, not per row --, reduces per job and
// combines into the job's 16-byte slot with 64-bit XOR atomics (exact, order-free).  The slots arrive zeroed with the call's upload.
// One launch per call whatever the number of jobs, levels, sizes and points; units are found in the group table by bisection.
//
// Level 0 (bits): a 64-bit word of the column is the lane mask of 64 row steps (pe_rows.hpp), lane l owns index 64 t + l (b >= 6) or
// l mod 2^b with 2^(6-b) rows in a word (b < 6).  Levels >= 3: threads over (index, a slice of the rows) with the subfield product.
// The epilogue's full product is mul_bytes: 16 byte steps under rolled loops (15 shifts of the basis, mul_walk<3> per byte), which
// keeps the register allocation of the bit path at four workgroups per CU.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "ctable.hpp"
#include "gf128.hpp"
#include "internal.hpp"
#include "pe_rows.hpp"

namespace bn {

namespace {

constexpr uint32_t kMeStage = 1u << kPeLogVecChunk;

// a * b: b = sum_k 2^(8k) * byte_k with byte_k in T_3 (the monomials of X_0..X_2 and of X_3..X_6 multiply without reduction)
__device__ __forceinline__ f128 mul_bytes(f128 a, f128 b)
{
	f128 r = f128_zero();
#pragma unroll 1
	for (uint32_t k6 = 0; k6 < 2; k6++) {
		const f128 a6 = k6 ? mulx<6>(a) : a;
		const uint64_t w = k6 ? b.hi : b.lo;
#pragma unroll 1
		for (uint32_t k = 0; k < 8; k++) {
			f128 x = a6;
			if (k & 1) x = mulx<3>(x);
			if (k & 2) x = mulx<4>(x);
			if (k & 4) x = mulx<5>(x);
			r ^= mul_walk<3>(x, (w >> (8 * k)) & 0xFFu);
		}
	}
	return r;
}

__device__ __forceinline__ void lds_xor(uint4 *slot, uint4 v)
{
	const unsigned long long lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32), hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
	unsigned long long *o = reinterpret_cast<unsigned long long *>(slot);
	if (lo) atomicXor(o, lo);
	if (hi) atomicXor(o + 1, hi);
}

// XOR over the 64 lanes of a wave (every lane active), the result in every lane
__device__ __forceinline__ uint4 wave_xor(uint4 v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		v.x ^= (uint32_t)__shfl_xor((int)v.x, d);
		v.y ^= (uint32_t)__shfl_xor((int)v.y, d);
		v.z ^= (uint32_t)__shfl_xor((int)v.z, d);
		v.w ^= (uint32_t)__shfl_xor((int)v.w, d);
	}
	return v;
}

// level 0: rows [j0, j0 + ch) of a bit column with 2^b indices; lvec holds hi[j0 .. j0 + ch)
__device__ __forceinline__ void me_bits(const uint64_t *__restrict__ evals, uint4 *accs, uint32_t b, uint64_t j0, uint32_t ch, const uint4 *lvec)
{
	const uint32_t lane = threadIdx.x & 63, wave = uni32(threadIdx.x >> 6);
	const uint32_t T = b > 6 ? 1u << (b - 6) : 1u; // words per row
	const uint32_t sh = b < 6 ? 6 - b : 0;         // log2 of the rows per word
	const uint32_t S = ch >> sh;                   // steps of the stage: rows (b >= 6) or words (b < 6); ch >= 2^sh (host)
	const uint64_t g0 = b >= 6 ? j0 << (b - 6) : j0 >> sh;
	const uint32_t sub = lane >> b;                // the lane's row inside a word (b < 6), else 0
	const uint32_t own = b < 6 ? lane & ((1u << b) - 1) : lane;
	if (wave * 64 >= S) return;
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
		lds_xor(accs + t * 64 + own, acc);
	}
}

// levels >= 3: thread (i, slice) sums its slice of the rows [j0, j0 + ch)
template <int IOTA>
__device__ __noinline__ void me_field(const uint64_t *__restrict__ evals, uint4 *accs, uint32_t b, uint64_t j0, uint32_t ch, const uint4 *lvec)
{
	const uint32_t n_out = 1u << b, P = n_out < 256 ? n_out : 256u;
	const uint32_t slice = threadIdx.x / P, n_slices = 256 / P;
	if (slice >= ch) return;
	for (uint32_t t = 0; t < n_out / P; t++) {
		const uint32_t i = t * P + (threadIdx.x & (P - 1));
		f128 acc = f128_zero();
		for (uint32_t j = slice; j < ch; j += n_slices) acc ^= pe_mul<IOTA>(to_f128(lvec[j]), evals, ((j0 + j) << b) + i);
		lds_xor(accs + i, to_u4(acc));
	}
}

} // namespace

// BITS_ONLY: every group of the launch is at level 0 (the instantiation without the subfield products of the row loop).
template <bool BITS_ONLY>
__global__ __launch_bounds__(256, BITS_ONLY ? 4 : 2) void k_mle_eval(const me_group *__restrict__ groups, uint32_t n_groups, const me_job *__restrict__ jobs)
{
	__shared__ uint4 lvec[kMeStage];
	__shared__ uint4 accs[kMeAccs];
	__shared__ uint4 sums[kMeGroupJobs];
	const me_group g = groups[find_job(groups, n_groups, blockIdx.x)];
	const uint32_t first = uni32(g.first), count = uni32(g.count), level = uni32(g.level), b = uni32(g.b), log_ch = uni32(g.log_ch);
	const uint4 *lo = (const uint4 *)uni64((uint64_t)g.lo), *hi = (const uint4 *)uni64((uint64_t)g.hi);
	const uint64_t r0 = (uint64_t)(blockIdx.x - uni32(g.start)) << log_ch;
	const uint64_t ch = (uint64_t)1 << log_ch;
	const uint32_t rows = ch < kMeStage ? (uint32_t)ch : kMeStage; // rows of a stage
	const uint32_t n_acc = count << b;                             // (<= kMeAccs: host)
	for (uint32_t e = threadIdx.x; e < n_acc; e += 256) accs[e] = uint4{0, 0, 0, 0};
	if (threadIdx.x < kMeGroupJobs) sums[threadIdx.x] = uint4{0, 0, 0, 0};
	for (uint64_t st = 0; st < ch; st += rows) {
		__syncthreads(); // (the readers of the previous stage are done; the cleared accumulators are visible)
		for (uint32_t e = threadIdx.x; e < rows; e += 256) lvec[e] = hi[r0 + st + e];
		__syncthreads();
		for (uint32_t c = 0; c < count; c++) {
			const uint64_t *evals = (const uint64_t *)uni64((uint64_t)jobs[first + c].evals);
			uint4 *acc_c = accs + (c << b);
			if constexpr (BITS_ONLY) {
				me_bits(evals, acc_c, b, r0 + st, rows, lvec);
			} else {
				switch (level) {
				case 0: me_bits(evals, acc_c, b, r0 + st, rows, lvec); break;
				case 3: me_field<3>(evals, acc_c, b, r0 + st, rows, lvec); break;
				case 4: me_field<4>(evals, acc_c, b, r0 + st, rows, lvec); break;
				case 5: me_field<5>(evals, acc_c, b, r0 + st, rows, lvec); break;
				case 6: me_field<6>(evals, acc_c, b, r0 + st, rows, lvec); break;
				default: me_field<7>(evals, acc_c, b, r0 + st, rows, lvec); break;
				}
			}
		}
	}
	__syncthreads();
	// ---- the epilogue: entry e = (job e >> b, index e mod 2^b); from b = 6 on a wave's 64 entries belong to one job
	for (uint32_t e = threadIdx.x; e < n_acc; e += 256) {
		const uint4 p = to_u4(mul_bytes(to_f128(accs[e]), to_f128(lo[e & ((1u << b) - 1)])));
		if (b >= 6) {
			const uint4 v = wave_xor(p);
			if ((threadIdx.x & 63) == 0) lds_xor(sums + (e >> b), v);
		} else {
			lds_xor(sums + (e >> b), p);
		}
	}
	__syncthreads();
	if (threadIdx.x < count) {
		const uint4 v = sums[threadIdx.x];
		const uint64_t v_lo = (uint64_t)v.x | ((uint64_t)v.y << 32), v_hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
		unsigned long long *o = reinterpret_cast<unsigned long long *>(jobs[first + threadIdx.x].slot);
		if (v_lo) atomicXor(o, (unsigned long long)v_lo);
		if (v_hi) atomicXor(o + 1, (unsigned long long)v_hi);
	}
}

// slots[j] -> rets[j] (the pinned result area; slot j belongs to the caller's job j), then the sequence word of the mailbox
__global__ __launch_bounds__(256) void k_me_publish(const f128 *__restrict__ slots, uint32_t n_jobs, f128 *rets, f128 *mail, uint64_t seq)
{
	for (uint32_t j = threadIdx.x; j < n_jobs; j += 256) {
		const f128 v = slots[j];
		__hip_atomic_store(&rets[j].lo, v.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		__hip_atomic_store(&rets[j].hi, v.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	}
	__threadfence_system();
	__syncthreads();
	if (threadIdx.x == 0) __hip_atomic_store(&mail[64].lo, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_mle_eval(hipStream_t s, const me_group *d_groups, uint32_t n_groups, const me_job *d_jobs, uint32_t total_units, bool bits_only)
{
	if (n_groups == 0 || total_units == 0) return hipSuccess;
	if (bits_only)
		hipLaunchKernelGGL(k_mle_eval<true>, dim3(total_units), dim3(256), 0, s, d_groups, n_groups, d_jobs);
	else
		hipLaunchKernelGGL(k_mle_eval<false>, dim3(total_units), dim3(256), 0, s, d_groups, n_groups, d_jobs);
	return hipGetLastError();
}

hipError_t launch_me_publish(hipStream_t s, const f128 *d_slots, uint32_t n_jobs, f128 *d_rets, f128 *d_mail, uint64_t seq)
{
	hipLaunchKernelGGL(k_me_publish, dim3(1), dim3(256), 0, s, d_slots, n_jobs, d_rets, d_mail, seq);
	return hipGetLastError();
}

} // namespace bn
