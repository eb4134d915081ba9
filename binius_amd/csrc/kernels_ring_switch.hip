// binius_amd/csrc/kernels_ring_switch.hip -- every ring-switch equality indicator of a call in one launch (RingSwitchEqInd::
// multilinear_extension, core/src/ring_switch/eq_ind.rs:81-147): for job j with query table Q (the tensor expansion of the claim's suffix),
// mixing coefficient m, kappa and the row-batch coefficients c
//   out_j[x] = sum_{i < 2^kappa} c[i] * limb_i(m * Q[x]),
// limb_i the i-th 2^(7 - kappa)-bit limb of a 128-bit element: what fill, tensor_expand(0, suffix) and fold_right over the subfield
// slice write, since tensor_expand from evals[0] = m is m times the expansion from 1.
//
// e -> sum_i c[i] * limb_i(m * e) is GF(2)-linear on the 16-byte element, so it is ONE nibble table of the ctable.hpp shape per job
// (32 x 16 x 16 B = 8 KiB, every table a 256-byte LDS bank row: the lookups are conflict-free whatever the data).  The basis entry of
// bit b is the image of m * 2^b (mul_basis) under the limb map: for kappa = 7 the XOR of the c[i] whose bit is set, for the other
// levels 2^kappa subfield-by-F products, which the kernel takes bit by bit as well: c[i] * s = XOR over the bits j of s of c[i] * 2^j,
// so with G[i * 2^(7 - kappa) + j] = c[i] * 2^j (128 elements that depend on kappa alone, one mul_basis of gf128.hpp each, rebuilt only
// when the next job of the run has another kappa) the image of e is the XOR of the G[t] whose bit t is set in e, at every kappa.
// Two neighbouring lanes share one basis entry, one per 64-bit word of m * 2^b, and combine with one lane exchange.
//
// The host sorts the jobs by query and cuts them into RUNS of up to kRsRunJobs jobs of one query.  A unit (one workgroup) is a run
// and a span of tiles of kRsTile elements of its query: the coefficients are staged once, the tables of the run's jobs are built once
// and stay in LDS (8 x 8 KiB + 4 KiB: two workgroups per CU), each tile is loaded ONCE into registers (eight elements per thread,
// thread t owning base + t + 256 q: the 16-byte loads and stores of a wave are contiguous) and taken through every table of the run.
// A query with more jobs than one run has further runs over the same tiles in the same launch: their reads come from cache.  An
// element beyond the query's end re-reads the tile's first element and is not stored: neither loads nor lookups are under a branch.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "ctable.hpp"
#include "gf128.hpp"
#include "internal.hpp"

namespace bn {

namespace {

// After every ctable_lookup: pins the schedule (left alone, the scheduler hoists the lookups of all the elements to the front and spills).
__device__ __forceinline__ void rs_pin(uint4 &acc) { asm volatile("" : "+v"(acc.x), "+v"(acc.y), "+v"(acc.z), "+v"(acc.w)::"memory"); }

// The XOR of the G[i] whose bit i is set in `word`, i < 64
__device__ __forceinline__ uint4 rs_masked_xor(const uint4 *__restrict__ G, uint64_t word)
{
	uint4 acc{0, 0, 0, 0};
	const uint32_t w[2] = {(uint32_t)word, (uint32_t)(word >> 32)};
#pragma unroll
	for (int half = 0; half < 2; half++) {
#pragma unroll 4
		for (int i = 0; i < 32; i++) {
			const uint32_t m = 0u - ((w[half] >> i) & 1u);
			const uint4 g = G[32 * half + i];
			acc.x ^= g.x & m;
			acc.y ^= g.y & m;
			acc.z ^= g.z & m;
			acc.w ^= g.w & m;
		}
	}
	return acc;
}

} // namespace

__global__ __launch_bounds__(256, 2) void k_ring_switch_eq_ind(const rs_run *__restrict__ runs, uint32_t n_runs, const rs_job *__restrict__ jobs,
                                                                const uint4 *__restrict__ coeffs, uint32_t n_staged, uint32_t span)
{
	extern __shared__ uint4 rs_lds[];
	uint4 *T = rs_lds;                     // kRsRunJobs tables of 512 entries
	uint4 *C = rs_lds + kRsRunJobs * 512;  // 128 coefficients
	uint4 *G = C + 128;                    // 128 bit images of the current kappa
	const uint32_t tid = threadIdx.x;
	const uint32_t u = blockIdx.x;
	const rs_run &run = runs[find_job(runs, n_runs, u)];
	const uint4 *query = (const uint4 *)uni64((uint64_t)run.query);
	const uint64_t len = uni64(run.len);
	const uint32_t first = uni32(run.first_job), nj = uni32(run.n_jobs);
	const uint64_t tile0 = (uint64_t)(u - uni32(run.start)) * span;

	if (tid < 128) C[tid] = tid < n_staged ? coeffs[tid] : uint4{0, 0, 0, 0};
	__syncthreads();
	// the basis entries (1, 2, 4, 8 of every table), then the other twelve as their XORs
	const uint32_t b = tid >> 1, h = tid & 1;
	uint32_t built = ~0u; // kappa of G
#pragma unroll 1
	for (uint32_t r = 0; r < nj; r++) {
		const rs_job &jb = jobs[first + r];
		const uint32_t kappa = uni32(jb.kappa);
		if (kappa != built) {
			__syncthreads(); // (the readers of the previous G are done)
			if (tid < 128) {
				const uint32_t iota = 7 - kappa;
				G[tid] = to_u4(mul_basis(to_f128(C[tid >> iota]), tid & ((1u << iota) - 1u)));
			}
			__syncthreads();
			built = kappa;
		}
		const f128 e = mul_basis(f128{uni64(jb.mixing.lo), uni64(jb.mixing.hi)}, b);
		uint4 v = rs_masked_xor(G + 64 * h, h ? e.hi : e.lo);
		v.x ^= __shfl_xor(v.x, 1);
		v.y ^= __shfl_xor(v.y, 1);
		v.z ^= __shfl_xor(v.z, 1);
		v.w ^= __shfl_xor(v.w, 1);
		if (h == 0) T[r * 512 + (b >> 2) * 16 + (1u << (b & 3))] = v;
	}
	__syncthreads();
	for (uint32_t i = tid; i < nj * 512; i += 256) {
		const uint32_t e = i & 15;
		if (e && !(e & (e - 1))) continue; // (a basis entry)
		T[i] = ctable_entry<true>(T + (i & ~15u), e);
	}
	__syncthreads();

#pragma unroll 1
	for (uint32_t t = 0; t < span; t++) {
		const uint64_t base = (tile0 + t) * kRsTile;
		if (base >= len) break;
		uint4 x[8];
#pragma unroll
		for (int q = 0; q < 8; q++) {
			const uint64_t idx = base + tid + 256u * q;
			x[q] = query[idx < len ? idx : base];
		}
#pragma unroll 1
		for (uint32_t r = 0; r < nj; r++) {
			uint4 *out = (uint4 *)uni64((uint64_t)jobs[first + r].out);
			const char *Tr = reinterpret_cast<const char *>(T + r * 512);
#pragma unroll
			for (int q = 0; q < 8; q++) {
				uint4 acc{0, 0, 0, 0};
				ctable_lookup<8>(acc, Tr, x[q].x);
				rs_pin(acc);
				ctable_lookup<8>(acc, Tr + 2048, x[q].y);
				rs_pin(acc);
				ctable_lookup<8>(acc, Tr + 4096, x[q].z);
				rs_pin(acc);
				ctable_lookup<8>(acc, Tr + 6144, x[q].w);
				rs_pin(acc);
				const uint64_t idx = base + tid + 256u * q;
				if (idx < len) out[idx] = acc;
			}
		}
	}
}

hipError_t launch_ring_switch_eq_ind(hipStream_t s, const rs_run *d_runs, uint32_t n_runs, const rs_job *d_jobs, const void *d_coeffs, uint32_t n_staged,
                                     uint32_t span, uint32_t total_units)
{
	if (n_runs == 0 || total_units == 0) return hipSuccess;
	constexpr size_t lds = (size_t)(kRsRunJobs * 512 + 256) * 16;
	const hipError_t attr = func_lds_limit(reinterpret_cast<const void *>(&k_ring_switch_eq_ind), (int)lds);
	if (attr != hipSuccess) return attr;
	hipLaunchKernelGGL(k_ring_switch_eq_ind, dim3(total_units), dim3(256), lds, s, d_runs, n_runs, d_jobs, (const uint4 *)d_coeffs, n_staged, span);
	return hipGetLastError();
}

} // namespace bn
