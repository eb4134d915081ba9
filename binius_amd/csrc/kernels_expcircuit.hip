// binius_amd/csrc/kernels_expcircuit.hip -- every layer of a batch of exponentiation circuits: the witness of the GKR exponentiation
// argument (core/src/protocols/gkr_exp/witness.rs:31-110 the static base, :139-156, 258-284 the dynamic base):
//   static :  V_0[i] = e_0[i] ? g : 1              V_k[i] = V_{k-1}[i]   * (e_k[i] ? g^(2^k) : 1)
//   dynamic:  V_0[i] = e_{w-1}[i] ? base[i] : 1    V_k[i] = V_{k-1}[i]^2 * (e_{w-1-k}[i] ? base[i] : 1)
// The e_j are bit columns read as bits (bit i = bit i & 31 of 32-bit word i >> 5); the g^(2^k) are host scalars.
//
// The independence used: row i of layer k depends on row i of layer k - 1 and on nothing else.  A wave owns a run of 224 rows
// (one wave-batch of the bit-sliced product, mul9_wave.hpp) and takes it through ALL layers of its witness, so a call is one
// launch whatever the widths; a job table found by bisection (one job per witness, as in kernels_prodtree.hip) lets that
// launch serve every witness of the batch.  Per layer the wave stages its two operands in LDS -- V_{k-1} (squared on the way
// for a dynamic base: squaring is GF(2)-linear, gf128.hpp square_tower, no product) and the select e ? c : 1 -- and runs one
// wave-batch over them, which stores V_k to the arena; the next layer reads it back from there (ordered by a device-scope fence
// pair: the rows were stored by other lanes of the same wave).  Layer 0 is the select alone.  Waves never wait for each other.
//
// k_bits_to_b128: dst[i] = bit i ? ONE : ZERO, the bit columns as B128 multilinears for the prover's sumchecks.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "gf128.hpp"
#include "internal.hpp"
#include "mul9_wave.hpp"

namespace bn {

namespace {

static_assert(kWB == (int)kExpRun, "units are planned on the host");
constexpr unsigned kStageQ4 = 2 * kWB;                 // the two staged operands of a wave, 224 elements each
constexpr unsigned kExpWaveQ4 = kWaveQ4 + kStageQ4;    // 576 + 448 uint4 = 16 KiB per wave

__device__ __forceinline__ uint4 sel_one(bool bit, uint4 c)
{
	return bit ? c : uint4{1, 0, 0, 0};
}

} // namespace

// Unit u (one per wave, four per workgroup, grid-stride): rows [r0, r0 + 224) of job j, r0 = (u - start) * 224.
__global__ __launch_bounds__(256, 2) void k_expcircuit(const expc_job *__restrict__ jobs, uint32_t n_jobs, uint32_t total_units)
{
	extern __shared__ uint4 tile[];
	// (the wave's index in a scalar register: see k_prodtree_big)
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	uint4 *const stage_a = tile + wave * kExpWaveQ4 + kWaveQ4, *const stage_b = stage_a + kWB;
	mul9_wave<1> mw;
	mw.init(tile + wave * kExpWaveQ4);
	for (uint32_t u = blockIdx.x * 4 + wave; u < total_units; u += gridDim.x * 4) {
		const expc_job &jb = jobs[find_job(jobs, n_jobs, u)];
		// (uniform per wave: into scalar registers)
		const uint32_t width = uni32(jb.width);
		const bool dynamic = uni32(jb.dynamic) != 0;
		const uint32_t start = uni32(jb.start);
		const uint64_t rows = uni64(jb.rows);
		const uint32_t *const *bits = (const uint32_t *const *)uni64((uint64_t)jb.bits);
		const uint4 *base = (const uint4 *)uni64((uint64_t)jb.base);
		uint4 *arena = (uint4 *)uni64((uint64_t)jb.arena);
		const uint64_t r0 = (uint64_t)(u - start) * kWB;
		const uint32_t cnt = rows - r0 < (uint64_t)kWB ? (uint32_t)(rows - r0) : (uint32_t)kWB; // (r0 < rows: the host plans ceil(rows / 224) units)
		// layer 0: the select alone
		{
			const uint32_t *col = (const uint32_t *)uni64((uint64_t)bits[dynamic ? width - 1 : 0]);
#pragma unroll 1
			for (uint32_t e = lane; e < cnt; e += 64) {
				const uint64_t row = r0 + e;
				const bool bit = (col[row >> 5] >> (row & 31)) & 1;
				arena[row] = sel_one(bit, dynamic ? base[row] : base[0]);
			}
		}
#pragma unroll 1
		for (uint32_t k = 1; k < width; k++) {
			// (layer k - 1 was stored by other lanes of this wave)
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
			const uint32_t *col = (const uint32_t *)uni64((uint64_t)bits[dynamic ? width - 1 - k : k]);
			const uint4 *prev = arena + (uint64_t)(k - 1) * rows;
#pragma unroll 1
			for (uint32_t e = lane; e < cnt; e += 64) {
				const uint64_t row = r0 + e;
				const bool bit = (col[row >> 5] >> (row & 31)) & 1;
				uint4 v = prev[row];
				if (dynamic) {
					const f128 sq = square_tower(f128{(uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32)});
					v = uint4{(uint32_t)sq.lo, (uint32_t)(sq.lo >> 32), (uint32_t)sq.hi, (uint32_t)(sq.hi >> 32)};
				}
				stage_a[e] = v;
				stage_b[e] = sel_one(bit, dynamic ? base[row] : base[k]);
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			// one wave-batch over the staged operands: elements 0 .. cnt - 1, stored to rows r0 .. of layer k
			mw.batch((const uint32_t *)stage_a, (const uint32_t *)stage_b, (uint32_t *)(arena + (uint64_t)k * rows + r0), 0, cnt);
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // (the stage is rewritten by the next layer)
			__builtin_amdgcn_wave_barrier();
		}
	}
}

__global__ __launch_bounds__(256) void k_bits_to_b128(const bits_job *__restrict__ jobs, uint32_t n_jobs)
{
	const bits_job &jb = jobs[find_job(jobs, n_jobs, blockIdx.x)];
	const uint64_t i = (uint64_t)(blockIdx.x - jb.start) * 256 + threadIdx.x;
	if (i < jb.rows) ((uint4 *)jb.dst)[i] = uint4{(jb.src[i >> 5] >> (i & 31)) & 1u, 0, 0, 0};
}

hipError_t launch_expcircuit(hipStream_t s, int n_cu, const expc_job *d_jobs, uint32_t n_jobs, uint32_t total_units)
{
	if (n_jobs == 0 || total_units == 0) return hipSuccess;
	constexpr size_t lds = (size_t)4 * kExpWaveQ4 * sizeof(uint4); // 64 KiB: two workgroups per CU
	const hipError_t attr = func_lds_limit(reinterpret_cast<const void *>(&k_expcircuit), (int)lds);
	if (attr != hipSuccess) return attr;
	const uint32_t wgs = (total_units + 3) / 4, cap = (uint32_t)n_cu * 2; // two workgroups per CU = two waves per SIMD
	hipLaunchKernelGGL(k_expcircuit, dim3(wgs < cap ? wgs : cap), dim3(256), lds, s, d_jobs, n_jobs, total_units);
	return hipGetLastError();
}

hipError_t launch_bits_to_b128(hipStream_t s, const bits_job *d_jobs, uint32_t n_jobs, uint32_t total_blocks)
{
	if (n_jobs == 0 || total_blocks == 0) return hipSuccess;
	hipLaunchKernelGGL(k_bits_to_b128, dim3(total_blocks), dim3(256), 0, s, d_jobs, n_jobs);
	return hipGetLastError();
}

} // namespace bn
