// binius_amd/csrc/kernels_mul9.hip -- element-wise GF(2^128) products, bit-sliced:
//   out[i] = a[i * a_stride] * b[b_off + i * b_stride]
// used by compute_composite for product compositions (crates/compute/src/layer.rs:459),
// pairwise_product_reduce (layer.rs:505: a = in, strides 2, b_off 1) and as the first step of the
// MLE-check round evaluation (b * eq, then the bivariate kernel).
//
// Same wave mapping as kernels_roundeval9.hip -- 7 groups of 9 lanes, each lane owning one of the 9
// GF(2^32) limb-combination products of two Karatsuba levels -- but here the products are needed per
// element, so after the multiplication the 9 partial products are exchanged through LDS, four lanes
// per group rebuild the four 32-bit limbs of the result in the bit-sliced domain
//     R0 = p0+p1+p3+p4                         R1 = p0+..+p5 + α(p1+p4)
//     R2 = p0+p1+p5+p6+p7 + α(p4)              R3 = p0+p1+p2+p5+p6+p7+p8 + α(p1+p3+p5+p7) + α²(p4)
// (α = multiplication by X_4 on 32 planes: pure XOR; derived from
// pairwise_recursive_arithmetic.rs:18-28 applied at levels 6 and 7), transpose them back
// (the 32x32 bit transpose is an involution) and store one word column each.
// A register carries 32 elements (no [1|inf] packing); a wave-batch is 7 x 32 = 224 elements.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "batch.hpp"
#include "bitslice.hpp"
#include "internal.hpp"
#include "mul9_wave.hpp"

namespace bn {

// The wave-batches wave_global, wave_global + n_waves, ... of one element-wise product; wt = this wave's LDS tile.
template <int STRIDE>
__device__ __forceinline__ void mul9_batches(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out,
                                             uint64_t n, uint64_t wave_global, uint64_t n_waves, uint4 *wt)
{
	mul9_wave<STRIDE> mw;
	mw.init(wt);
	const uint64_t n_batches = (n + kWB - 1) / kWB;
	for (uint64_t bt = wave_global; bt < n_batches; bt += n_waves)
		mw.batch(a, b, out, bt * kWB, n);
}

template <int STRIDE>
__global__ __launch_bounds__(256, 2) void k_mul9_dual(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                     uint32_t *__restrict__ out, uint64_t n)
{
	extern __shared__ uint4 tile2[];
	const unsigned wave = threadIdx.x >> 6;
	mul9_wave<STRIDE> mw;
	mw.init(tile2 + wave * 2 * kWaveQ4);
	if ((threadIdx.x & 63) < kQ)
		tile2[wave * 2 * kWaveQ4 + kWaveQ4 + kZero * kQ + (threadIdx.x & 63)] = uint4{0, 0, 0, 0}; // the second region's zero block
	const uint64_t n_steps = (n + 2 * kWB - 1) / (2 * kWB);
	const uint64_t n_waves = (uint64_t)gridDim.x * 4;
	for (uint64_t st = (uint64_t)blockIdx.x * 4 + wave; st < n_steps; st += n_waves)
		mw.batch2(a, b, out, st * 2 * kWB, n);
}

template <int STRIDE>
__global__ __launch_bounds__(256, 2) void k_mul9(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                uint32_t *__restrict__ out, uint64_t n)
{
	__shared__ uint4 tile[4][kWaveQ4];
	const unsigned wave = threadIdx.x >> 6;
	mul9_batches<STRIDE>(a, b, out, n, (uint64_t)blockIdx.x * 4 + wave, (uint64_t)gridDim.x * 4, tile[wave]);
}

// Several levels of pairwise_product_reduce in one launch: a workgroup takes 4 adjacent wave-batches of the first level
// (896 products), and -- their results being exactly the inputs of the 448 products under them -- goes on with 2 batches of
// the next level, 1 of the third, half a batch of the fourth, before it moves to its next 896.  What a level reads was
// stored by waves of the same workgroup (same CU, same L1: a workgroup barrier orders it); no launch between the levels
// and no grid-wide dependency.  Level l (0-based) reads lv[l - 1] (level 0: in) and writes lv[l]; n0 = products of level 0.
__global__ __launch_bounds__(256, 2) void k_mul9_tree(mul9_tree_args args)
{
	__shared__ uint4 tile[4][kWaveQ4];
	const unsigned wave = threadIdx.x >> 6;
	mul9_wave<2> mw;
	mw.init(tile[wave]);
	constexpr uint64_t kSB = 4 * kWB; // products of the first level per workgroup step
	const uint64_t n_sb = (args.n0 + kSB - 1) / kSB;
	for (uint64_t k = blockIdx.x; k < n_sb; k += gridDim.x) {
		for (uint32_t l = 0; l < args.n_levels; l++) {
			if (l) __syncthreads();
			const uint64_t span = kSB >> l;           // products of level l under this step
			const uint64_t n_l = args.n0 >> l;        // products of level l in all
			const uint64_t e0 = span * k + (uint64_t)kWB * wave;
			uint64_t limit = span * (k + 1);
			if (limit > n_l) limit = n_l;
			if (e0 < limit) {
				const uint32_t *src = l ? args.lv[l - 1] : args.in;
				mw.batch(src, src + 4, args.lv[l], e0, limit);
			}
		}
		__syncthreads(); // (the LDS tiles are per wave, but the next step's first level must not overtake a wave still reading)
	}
}

// n_jobs products of n elements each in one launch: wave-batches are dealt out over (job, batch) pairs; a wave's job pointers are
// read from the table (pinned memory) and held in scalar registers
__global__ __launch_bounds__(256, 2) void k_mul9_jobs(const mul9_job *__restrict__ jobs, uint32_t n_jobs, uint64_t n)
{
	__shared__ uint4 tile[4][kWaveQ4];
	const unsigned wave = threadIdx.x >> 6;
	mul9_wave<1> mw;
	mw.init(tile[wave]);
	const uint64_t per_job = (n + kWB - 1) / kWB, total = per_job * n_jobs;
	const uint64_t n_waves = (uint64_t)gridDim.x * 4;
	// (the table is pinned host memory: a wave reads a job's pointers once, when it moves on to that job)
	uint32_t cur = ~0u;
	const uint32_t *a = nullptr, *b = nullptr, *a2 = nullptr, *b2 = nullptr;
	uint32_t *out = nullptr;
	for (uint64_t bt = (uint64_t)blockIdx.x * 4 + wave; bt < total; bt += n_waves) {
		const uint32_t j = (uint32_t)(bt / per_job);
		const uint64_t e0 = (bt - (uint64_t)j * per_job) * kWB;
		if (j != cur) {
			cur = j; // (uniform per wave: the pointers into scalar registers)
			a = (const uint32_t *)uni64((uint64_t)jobs[j].a);
			b = (const uint32_t *)uni64((uint64_t)jobs[j].b);
			out = (uint32_t *)uni64((uint64_t)jobs[j].out);
			a2 = (const uint32_t *)uni64((uint64_t)jobs[j].a2);
			b2 = (const uint32_t *)uni64((uint64_t)jobs[j].b2);
		}
		mw.batch(a, b, out, e0, n, a2, b2);
	}
}

// the same with two wave-batches per rebuild (batch2: a fifth fewer instructions per product), for launches with more batches than
// wave slots
__global__ __launch_bounds__(256, 2) void k_mul9_jobs_dual(const mul9_job *__restrict__ jobs, uint32_t n_jobs, uint64_t n)
{
	extern __shared__ uint4 tile2[];
	const unsigned wave = threadIdx.x >> 6;
	mul9_wave<1> mw;
	mw.init(tile2 + wave * 2 * kWaveQ4);
	if ((threadIdx.x & 63) < kQ)
		tile2[wave * 2 * kWaveQ4 + kWaveQ4 + kZero * kQ + (threadIdx.x & 63)] = uint4{0, 0, 0, 0}; // the second region's zero block
	const uint64_t per_job = (n + 2 * kWB - 1) / (2 * kWB), total = per_job * n_jobs;
	const uint64_t n_waves = (uint64_t)gridDim.x * 4;
	uint32_t cur = ~0u;
	const uint32_t *a = nullptr, *b = nullptr, *a2 = nullptr, *b2 = nullptr;
	uint32_t *out = nullptr;
	for (uint64_t st = (uint64_t)blockIdx.x * 4 + wave; st < total; st += n_waves) {
		const uint32_t j = (uint32_t)(st / per_job);
		const uint64_t e0 = (st - (uint64_t)j * per_job) * 2 * kWB;
		if (j != cur) {
			cur = j;
			a = (const uint32_t *)uni64((uint64_t)jobs[j].a);
			b = (const uint32_t *)uni64((uint64_t)jobs[j].b);
			out = (uint32_t *)uni64((uint64_t)jobs[j].out);
			a2 = (const uint32_t *)uni64((uint64_t)jobs[j].a2);
			b2 = (const uint32_t *)uni64((uint64_t)jobs[j].b2);
		}
		mw.batch2(a, b, out, e0, n, a2, b2);
	}
}

hipError_t launch_mul9_jobs(hipStream_t s, int n_cu, const mul9_job *d_jobs, uint32_t n_jobs, uint64_t n)
{
	if (n_jobs == 0 || n == 0) return hipSuccess;
	const uint64_t total = ((n + kWB - 1) / kWB) * n_jobs;
	uint64_t blocks = (total + 3) / 4;
	const uint64_t cap = (uint64_t)n_cu * 2;
	if (blocks > cap) blocks = cap;
	__atomic_thread_fence(__ATOMIC_SEQ_CST); // (the table is in memory before the doorbell rings)
	if (total > cap * 4) {
		constexpr size_t lds = (size_t)4 * 2 * kWaveQ4 * sizeof(uint4);
		const hipError_t attr1 = func_lds_limit(reinterpret_cast<const void *>(&k_mul9_jobs_dual), (int)lds);
		if (attr1 != hipSuccess) return attr1;
		const uint64_t steps = ((n + 2 * kWB - 1) / (2 * kWB)) * n_jobs;
		uint64_t blk = (steps + 3) / 4;
		if (blk > cap) blk = cap;
		hipLaunchKernelGGL(k_mul9_jobs_dual, dim3((unsigned)blk), dim3(256), lds, s, d_jobs, n_jobs, n);
		return hipGetLastError();
	}
	hipLaunchKernelGGL(k_mul9_jobs, dim3((unsigned)blocks), dim3(256), 0, s, d_jobs, n_jobs, n);
	return hipGetLastError();
}

hipError_t launch_mul9(hipStream_t s, int n_cu, const void *a, uint64_t a_stride, const void *b, uint64_t b_stride, uint64_t b_off,
                       void *out, uint64_t n)
{
	if (n == 0) return hipSuccess;
	const uint64_t n_batches = (n + kWB - 1) / kWB;
	uint64_t blocks = (n_batches + 3) / 4;
	const uint64_t cap = (uint64_t)n_cu * 2; // two workgroups per CU = two waves per SIMD
	if (blocks > cap) blocks = cap;
	const uint32_t *pb = (const uint32_t *)b + b_off * 4;
	// more batches than wave slots: two batches per rebuild (k_mul9_dual); BN_MUL9_DUAL=0 keeps the one-batch kernel
	static const bool dual_on = [] {
		const char *e = bn::settled_knob("BN_MUL9_DUAL");
		return !(e && e[0] == '0');
	}();
	// (unit strides only: the strided form -- one level of pairwise_product_reduce by itself -- never has that many batches
	// with the default level fusion, and a path the tests do not reach is not worth a fifth of its time)
	if (dual_on && n_batches > cap * 4 && a_stride == 1 && b_stride == 1) {
		constexpr size_t lds = (size_t)4 * 2 * kWaveQ4 * sizeof(uint4);
		const hipError_t attr1 = func_lds_limit(reinterpret_cast<const void *>(&k_mul9_dual<1>), (int)lds);
		if (attr1 != hipSuccess) return attr1;
		const uint64_t n_steps = (n_batches + 1) / 2;
		uint64_t blk = (n_steps + 3) / 4;
		if (blk > cap) blk = cap;
		hipLaunchKernelGGL(k_mul9_dual<1>, dim3((unsigned)blk), dim3(256), lds, s, (const uint32_t *)a, pb, (uint32_t *)out, n);
		return hipGetLastError();
	}
	if (a_stride == 1 && b_stride == 1)
		hipLaunchKernelGGL(k_mul9<1>, dim3((unsigned)blocks), dim3(256), 0, s, (const uint32_t *)a, pb, (uint32_t *)out, n);
	else if (a_stride == 2 && b_stride == 2)
		hipLaunchKernelGGL(k_mul9<2>, dim3((unsigned)blocks), dim3(256), 0, s, (const uint32_t *)a, pb, (uint32_t *)out, n);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

hipError_t launch_mul9_tree(hipStream_t s, int n_cu, const mul9_tree_args &args)
{
	if (args.n0 == 0 || args.n_levels == 0 || args.n_levels > 4) return hipErrorInvalidValue;
	uint64_t blocks = (args.n0 + 4 * kWB - 1) / (4 * kWB);
	const uint64_t cap = (uint64_t)n_cu * 2;
	if (blocks > cap) blocks = cap;
	hipLaunchKernelGGL(k_mul9_tree, dim3((unsigned)blocks), dim3(256), 0, s, args);
	return hipGetLastError();
}

} // namespace bn
