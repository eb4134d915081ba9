// binius_amd/csrc/kernels_prodtree.hip -- every layer of a batch of halves-product trees: the circuit of the GKR grand-product
// argument (core/src/protocols/gkr_gpa/gkr_gpa.rs:38-90, the same layers as prodcheck/prove.rs:24-77):
//   layer_j[i] = layer_{j+1}[i] * layer_{j+1}[i + 2^j],   0 <= i < 2^j,   layer_n = the input, elements past its length = ONE.
// A tree's layers live in one arena in heap order (layer j at arena + 2^j), so the two multilinears of layer j's sumcheck
// are the contiguous halves of layer j + 1.
//
// The independence used: for a fixed residue r mod 2^s, the elements {r + t 2^s} of layer s + T are a complete subtree
// down to element r of layer s.  Whoever owns a set of residues produces T layers from one read of layer s + T with no
// grid-wide dependency in between.  Two forms, both driven by a job table so that one launch serves every tree of a batch (a unit
// of batch.hpp is a workgroup of the small form, a run of the big one):
//
// * k_prodtree_big (layers above 2^15 elements): a workgroup owns a run of 448 contiguous residues (896 in the two-batch form of
//   the product); its four waves take the four wave-batches of the 2 x 448 products of the first layer (two chunks of 448
//   contiguous elements each, 2^s apart), two of them the 448 products under those.  The product is mul9_wave (kernels_mul9.hip: bit-sliced, 224 per wave-batch); what the
//   second layer reads was stored by waves of the same workgroup, ordered by a workgroup barrier -- the halves counterpart
//   of k_mul9_tree.  With one layer per job the run is twice as long.
// * k_prodtree_small (from 2^15 elements down, where a layer is one dependent chain whatever its size): a workgroup owns ONE
//   residue, gathers its 2^L <= 64 elements into LDS and walks L layers there with the lane-cooperative product of
//   kernels_pairtree.hip (groupmul.hpp), 8 .. 64 lanes per product as the layer empties; every layer is also stored to the
//   arena.  In LDS the subtree is again paired by halves.  The last six layers of a tree are one workgroup.
//
// Elements of a truncated input past its length are ONE: the small form substitutes it as it gathers; in the big form a
// product with ONE is a copy of the other operand (or ONE), done by the wave next to its bit-sliced batch.  Inputs are only read.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "gf128.hpp"
#include "groupmul.hpp"
#include "internal.hpp"
#include "mul9_wave.hpp"

namespace bn {

namespace {

constexpr uint32_t kSmallLogS = kProdtreeSmallLevels; // 2^6 elements per workgroup
constexpr uint32_t kSmallThreads = 256;
static_assert(kWB == (int)kProdtreeBatch, "run sizes are planned on the host");

// One layer inside a workgroup: product q = src[q] * src[q + n_prod], kept in LDS for the next layer and stored to the
// arena (element q of this residue's subtree lies q << s elements into the layer).
template <int G>
__device__ __forceinline__ void halves_level(const f128 *src, f128 *keep, f128 *__restrict__ gout, uint32_t s, unsigned n_prod)
{
	const unsigned q = threadIdx.x / G, j = threadIdx.x % G;
	if (q < n_prod) { // (whole groups)
		const f128 p = group_product<G>(src[q], src[q + n_prod], j);
		if (j == 0) {
			keep[q] = p;
			gout[(uint64_t)q << s] = p;
		}
	}
}

// as many lanes per product as the workgroup has for this layer (8 .. 64)
__device__ __forceinline__ void halves_level_any(const f128 *src, f128 *keep, f128 *gout, uint32_t s, unsigned n_prod)
{
	if (n_prod * 64 <= kSmallThreads)
		halves_level<64>(src, keep, gout, s, n_prod);
	else if (n_prod * 32 <= kSmallThreads)
		halves_level<32>(src, keep, gout, s, n_prod);
	else if (n_prod * 16 <= kSmallThreads)
		halves_level<16>(src, keep, gout, s, n_prod);
	else
		halves_level<8>(src, keep, gout, s, n_prod);
}

} // namespace

// Workgroup u of job j: residue r = u - start of the 2^s residues, s = m - n_levels; layers m - 1 .. s of its subtree.
__global__ __launch_bounds__(kSmallThreads) void k_prodtree_small(const prodtree_job *__restrict__ jobs, uint32_t n_jobs)
{
	__shared__ f128 buf[2][1u << kSmallLogS];
	const prodtree_job &jb = jobs[find_job(jobs, n_jobs, blockIdx.x)];
	const uint32_t m = jb.m, L = jb.n_levels, s = m - L;
	const uint64_t r = blockIdx.x - jb.start;
	const f128 *__restrict__ src = jb.src;
	f128 *__restrict__ arena = jb.arena;
	if (threadIdx.x < (1u << L)) {
		const uint64_t idx = ((uint64_t)threadIdx.x << s) + r;
		buf[0][threadIdx.x] = idx < jb.src_len ? src[idx] : f128_one();
	}
	__syncthreads();
	unsigned n_prod = 1u << (L - 1), cur = 0;
	for (uint32_t l = 1; l <= L; l++) {
		halves_level_any(buf[cur], buf[cur ^ 1], arena + ((uint64_t)1 << (m - l)) + r, s, n_prod);
		__syncthreads();
		n_prod >>= 1;
		cur ^= 1;
	}
}

// Run k of job j: residues [run * w, (run + 1) * w) of the 2^s, s = m - T; layers m - 1 .. s.  A wave's step is one wave-batch
// (224 products) or, DUAL, two batches with one rebuild (mul9_wave::batch2: a fifth fewer instructions per product, twice the
// latency per step -- for launches with more batches than wave slots, as in launch_mul9); w = 4 steps >> (T - 1).
template <bool DUAL>
__global__ __launch_bounds__(256, 2) void k_prodtree_big(const prodtree_job *__restrict__ jobs, uint32_t n_jobs, uint32_t total_runs)
{
	extern __shared__ uint4 tile[];
	constexpr unsigned kRegions = DUAL ? 2 : 1;
	constexpr uint64_t kStep = (uint64_t)kRegions * kWB;
	// (the wave's index in a scalar register: everything derived from it -- operand pointers, limits -- stays out of the vector
	// registers, which the product needs: 194 of 256 at two waves per SIMD)
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	mul9_wave<1> mw;
	mw.init(tile + wave * kRegions * kWaveQ4);
	if (DUAL && lane < kQ) tile[wave * 2 * kWaveQ4 + kWaveQ4 + kZero * kQ + lane] = uint4{0, 0, 0, 0}; // the second region's zero block
	for (uint32_t k = blockIdx.x; k < total_runs; k += gridDim.x) {
		const prodtree_job &jb = jobs[find_job(jobs, n_jobs, k)];
		// (uniform per workgroup: into scalar registers)
		const uint32_t m = uni32(jb.m), T = uni32(jb.n_levels);
		const uint32_t start = uni32(jb.start);
		const uint64_t src_len = uni64(jb.src_len);
		const f128 *src0 = (const f128 *)uni64((uint64_t)jb.src);
		f128 *arena = (f128 *)uni64((uint64_t)jb.arena);
		const uint32_t s = m - T;
		const uint64_t n_res = (uint64_t)1 << s;
		const uint32_t spc = 4u >> (T - 1); // wave steps per chunk of the run
		const uint64_t r0 = (uint64_t)(k - start) * spc * kStep;
		const uint64_t r1 = r0 + (uint64_t)spc * kStep < n_res ? r0 + (uint64_t)spc * kStep : n_res;
		const unsigned chunk = wave / spc, sub = wave % spc;
		for (uint32_t l = 0; l < T; l++) {
			if (l) __syncthreads(); // (the layer just stored is read back by other waves of this workgroup)
			// layer m - l -> layer m - l - 1: 2^(T - 1 - l) chunks of this run's residues
			const uint64_t half = (uint64_t)1 << (m - l - 1);
			const uint64_t e0 = r0 + (uint64_t)sub * kStep;
			if (chunk < (1u << (T - 1 - l)) && e0 < r1) {
				const uint64_t c_off = (uint64_t)chunk << s;
				const f128 *a = (l ? arena + 2 * half : src0) + c_off;
				f128 *out = arena + half + c_off;
				const uint64_t len = l ? 2 * half : src_len;
				// valid elements of the two operands, counted from the chunk: e < lb: a product; lb <= e < la: a copy; else ONE
				const uint64_t la = len > c_off ? len - c_off : 0, lb = len > c_off + half ? len - c_off - half : 0;
				const uint64_t plim = lb < r1 ? lb : r1;
				if (e0 < plim) {
					if constexpr (DUAL)
						mw.batch2((const uint32_t *)a, (const uint32_t *)(a + half), (uint32_t *)out, e0, plim);
					else
						mw.batch((const uint32_t *)a, (const uint32_t *)(a + half), (uint32_t *)out, e0, plim);
				}
				const uint64_t e1 = e0 + kStep < r1 ? e0 + kStep : r1;
				for (uint64_t e = (e0 > lb ? e0 : lb) + lane; e < e1; e += 64) {
					const uint4 one{1, 0, 0, 0};
					((uint4 *)out)[e] = e < la ? ((const uint4 *)a)[e] : one;
				}
			}
		}
		__syncthreads(); // (the next run's first layer must not overtake a wave still reading this one's)
	}
}

// out[t] = *srcs[t] (a tree's root: arena[1], or its single input element), ONE for a null pointer
__global__ void k_prodtree_roots(const f128 *const *__restrict__ srcs, uint32_t n, f128 *__restrict__ out)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < n) out[t] = srcs[t] ? *srcs[t] : f128_one();
}

// dst[i] = i < src_len ? src[i] : ONE for i < 2^m, every job of the table in one launch (start = first block of 256 elements)
__global__ __launch_bounds__(256) void k_prodtree_pad(const prodtree_job *__restrict__ jobs, uint32_t n_jobs)
{
	const prodtree_job &jb = jobs[find_job(jobs, n_jobs, blockIdx.x)];
	const uint64_t i = (uint64_t)(blockIdx.x - jb.start) * 256 + threadIdx.x;
	if (i < ((uint64_t)1 << jb.m)) {
		const uint4 one{1, 0, 0, 0};
		((uint4 *)jb.arena)[i] = i < jb.src_len ? ((const uint4 *)jb.src)[i] : one;
	}
}

hipError_t launch_prodtree_small(hipStream_t s, const prodtree_job *d_jobs, uint32_t n_jobs, uint32_t total_wgs)
{
	if (n_jobs == 0 || total_wgs == 0) return hipSuccess;
	hipLaunchKernelGGL(k_prodtree_small, dim3(total_wgs), dim3(kSmallThreads), 0, s, d_jobs, n_jobs);
	return hipGetLastError();
}

hipError_t launch_prodtree_big(hipStream_t s, int n_cu, const prodtree_job *d_jobs, uint32_t n_jobs, uint32_t total_runs, bool dual)
{
	if (n_jobs == 0 || total_runs == 0) return hipSuccess;
	const uint32_t cap = (uint32_t)n_cu * 2; // two workgroups per CU = two waves per SIMD
	const dim3 grid(total_runs < cap ? total_runs : cap);
	if (dual) {
		constexpr size_t lds = (size_t)4 * 2 * kWaveQ4 * sizeof(uint4);
		const hipError_t attr = func_lds_limit(reinterpret_cast<const void *>(&k_prodtree_big<true>), (int)lds);
		if (attr != hipSuccess) return attr;
		hipLaunchKernelGGL(k_prodtree_big<true>, grid, dim3(256), lds, s, d_jobs, n_jobs, total_runs);
	} else {
		hipLaunchKernelGGL(k_prodtree_big<false>, grid, dim3(256), (size_t)4 * kWaveQ4 * sizeof(uint4), s, d_jobs, n_jobs, total_runs);
	}
	return hipGetLastError();
}

hipError_t launch_prodtree_roots(hipStream_t s, const f128 *const *d_srcs, uint32_t n, f128 *d_out)
{
	if (n == 0) return hipSuccess;
	hipLaunchKernelGGL(k_prodtree_roots, dim3((n + 255) / 256), dim3(256), 0, s, d_srcs, n, d_out);
	return hipGetLastError();
}

hipError_t launch_prodtree_pad(hipStream_t s, const prodtree_job *d_jobs, uint32_t n_jobs, uint32_t total_blocks)
{
	if (n_jobs == 0 || total_blocks == 0) return hipSuccess;
	hipLaunchKernelGGL(k_prodtree_pad, dim3(total_blocks), dim3(256), 0, s, d_jobs, n_jobs);
	return hipGetLastError();
}

} // namespace bn
