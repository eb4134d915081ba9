// binius_amd/csrc/kernels_derive.hip -- the virtual columns of a constraint system built on the device from the columns they are
// functions of (MultilinearPolyVariant, multilinear.rs of core's oracle module; value by value: constraint_system/validate.rs:151-279 and
// math/src/fold.rs:27-77): every Shifted, Repeating, ZeroPadded and unit-coefficient LinearCombination column of a call in ONE launch.
//
// A streaming kernel: the inner column is read once, the output written once.  The host (abi_derive.cpp) turns every job into one of
// seven FORMS whose parameters are in bit coordinates (internal.hpp, derive_job), so one code path serves every tower level.  Jobs are
// sorted by first unit and found by bisection (batch.hpp); a unit (one workgroup) is kDeriveUnitElems contiguous 16-byte outputs of one
// job, taken in chunks of 1024 -- the lookup is paid once per unit --, thread t owning elements t, t + 256, ... of a chunk: every
// store instruction of a wave writes 1 KiB in one run.  A thread issues all loads of its four elements before it combines any of them.  Indices of elements past the job's end are clamped to its last element -- the
// loads stay inside the column and depend on no data -- and only the store is predicated.
// Plain 16-byte vector loads and stores, 64-bit element offsets throughout.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "internal.hpp"

namespace bn {

constexpr uint32_t kDvPerThread = 4;                          // elements a thread holds at a time
constexpr uint32_t kDvChunkElems = 256 * kDvPerThread;        // elements the workgroup handles at a time
constexpr uint32_t kDvChunks = kDeriveUnitElems / kDvChunkElems; // chunks of a unit, one after the other

// (a pointer out of the job table is a generic pointer to the compiler: say that it is device memory, for global instead of flat
// loads and stores)
typedef uint32_t derive_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 dv_gload(const void *p, uint64_t idx)
{
	const derive_u32x4 x = ((const __attribute__((address_space(1))) derive_u32x4 *)(uintptr_t)p)[idx];
	return uint4{x.x, x.y, x.z, x.w};
}
__device__ __forceinline__ void dv_gstore(uint4 *p, uint64_t idx, uint4 v)
{
	((__attribute__((address_space(1))) derive_u32x4 *)(uintptr_t)p)[idx] = derive_u32x4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ uint64_t dv_lo(uint4 v) { return (uint64_t)v.x | ((uint64_t)v.y << 32); }
__device__ __forceinline__ uint64_t dv_hi(uint4 v) { return (uint64_t)v.z | ((uint64_t)v.w << 32); }
__device__ __forceinline__ uint4 dv_pack(uint64_t lo, uint64_t hi) { return uint4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)}; }
__device__ __forceinline__ uint64_t dv_mask(uint32_t bits) { return bits >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << bits) - 1; }
// bits [r, r + 128) of the 256 bits b : a, r < 128 and the same in every lane
__device__ __forceinline__ uint4 dv_window(uint4 a, uint4 b, uint32_t r)
{
	const bool up = (r & 64) != 0;
	const uint32_t br = r & 63;
	const uint64_t w0 = up ? dv_hi(a) : dv_lo(a), w1 = up ? dv_lo(b) : dv_hi(a), w2 = up ? dv_hi(b) : dv_lo(b);
	if (br == 0) return dv_pack(w0, w1);
	return dv_pack((w0 >> br) | (w1 << (64 - br)), (w1 >> br) | (w2 << (64 - br)));
}

__global__ __launch_bounds__(256) void k_derive_columns(const derive_job *__restrict__ jobs, uint32_t n_jobs, const void *const *__restrict__ terms)
{
	const uint32_t tid = threadIdx.x, u = blockIdx.x;
	const derive_job &jb = jobs[find_job(jobs, n_jobs, u)];
	const void *in = (const void *)uni64((uint64_t)jb.in);
	uint4 *out = (uint4 *)uni64((uint64_t)jb.out);
	const uint64_t len = uni64(jb.out_elems), m0 = uni64(jb.m0), m1 = uni64(jb.m1);
	const uint32_t p0 = uni32(jb.p0), p1 = uni32(jb.p1), p2 = uni32(jb.p2), p3 = uni32(jb.p3), form = uni32(jb.form);
	const uint64_t unit_first = (uint64_t)(u - uni32(jb.start)) * kDeriveUnitElems;
#define DV_AT(q) (j[q] < len ? j[q] : len - 1)
#pragma unroll 1
	for (uint32_t c = 0; c < kDvChunks; c++) { // the unit, a chunk of 256 * kDvPerThread elements at a time: the job lookup above is paid once
		const uint64_t base = unit_first + c * kDvChunkElems + tid;
		if (base - tid >= len) break;
		uint64_t j[kDvPerThread]; // the element each store goes to; loads use the clamped index
		uint4 r[kDvPerThread];
#pragma unroll
		for (uint32_t q = 0; q < kDvPerThread; q++) j[q] = base + 256 * q;

		switch (form) {
		case kDvShiftWord: {
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) r[q] = dv_gload(in, DV_AT(q));
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) {
				const uint64_t lo = dv_lo(r[q]), hi = dv_hi(r[q]);
				r[q] = dv_pack(((lo << p0) & m0) | ((lo >> p1) & m1), ((hi << p0) & m0) | ((hi >> p1) & m1));
			}
			break;
		}
		case kDvShiftElem: {
			const uint64_t in_block = ((uint64_t)1 << p0) - 1;
			uint4 a[kDvPerThread], b[kDvPerThread];
			bool za[kDvPerThread], zb[kDvPerThread];
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) {
				const uint64_t at = DV_AT(q), e = at & in_block, blk = at - e, q0 = e + m0, q1 = q0 + 1;
				za[q] = !p1 && (q0 - m1) > in_block; // (unsigned: below m1 wraps to a large value)
				zb[q] = !p1 && (q1 - m1) > in_block;
				a[q] = dv_gload(in, blk + (q0 & in_block));
				b[q] = dv_gload(in, blk + (q1 & in_block));
			}
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) {
				const uint4 zero{0, 0, 0, 0};
				r[q] = dv_window(za[q] ? zero : a[q], zb[q] ? zero : b[q], p2);
			}
			break;
		}
		case kDvRepeat: {
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) r[q] = dv_gload(in, DV_AT(q) & m0);
			if (p0) {
#pragma unroll
				for (uint32_t q = 0; q < kDvPerThread; q++) {
					uint64_t w = dv_lo(r[q]) & dv_mask(p0);
					for (uint32_t b = p0; b < 64; b <<= 1) w |= w << b;
					r[q] = dv_pack(w, w);
				}
			}
			break;
		}
		case kDvPadElem: {
			const uint64_t in_run = ((uint64_t)1 << p0) - 1, in_period = ((uint64_t)1 << p1) - 1;
			bool z[kDvPerThread];
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) {
				const uint64_t at = DV_AT(q), c = at & in_period;
				z[q] = (c >> p0) != m0;
				r[q] = dv_gload(in, ((at >> p1) << p0) + (c & in_run));
			}
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++)
				if (z[q]) r[q] = uint4{0, 0, 0, 0};
			break;
		}
		case kDvPadField: {
			const uint64_t in_period = ((uint64_t)1 << p1) - 1, field = dv_mask(1u << p0);
			uint32_t so[kDvPerThread];
			bool z[kDvPerThread];
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) {
				const uint64_t at = DV_AT(q), sb = (at >> p1) << p0;
				z[q] = (at & in_period) != m0;
				so[q] = (uint32_t)sb & 127;
				r[q] = dv_gload(in, sb >> 7);
			}
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) {
				const uint64_t v = z[q] ? 0 : (((so[q] & 64) ? dv_hi(r[q]) : dv_lo(r[q])) >> (so[q] & 63)) & field;
				r[q] = (p2 & 64) ? dv_pack(0, v << (p2 & 63)) : dv_pack(v << (p2 & 63), 0);
			}
			break;
		}
		case kDvPadSpread: {
			const uint32_t take = 64u >> p2, runs = 64u >> p1;
			const uint64_t run = dv_mask(1u << p0), taken = dv_mask(take);
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) r[q] = dv_gload(in, DV_AT(q) >> p2);
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) {
				uint64_t w[2];
#pragma unroll
				for (uint32_t h = 0; h < 2; h++) {
					const uint64_t W = 2 * DV_AT(q) + h, sw = W >> p2; // the output word, the inner word it is made of
					const uint64_t f = (((sw & 1) ? dv_hi(r[q]) : dv_lo(r[q])) >> ((uint32_t)(W & dv_mask(p2)) * take)) & taken;
					uint64_t o = 0;
					for (uint32_t k = 0; k < runs; k++) o |= ((f >> (k << p0)) & run) << ((k << p1) + p3);
					w[h] = o;
				}
				r[q] = dv_pack(w[0], w[1]);
			}
			break;
		}
		default: { // kDvXor
			const uint32_t first = uni32(jb.first_term), n_terms = uni32(jb.n_terms);
			uint64_t at[kDvPerThread];
#pragma unroll
			for (uint32_t q = 0; q < kDvPerThread; q++) {
				at[q] = DV_AT(q);
				r[q] = dv_pack(m0, m1);
			}
#pragma unroll 1
			for (uint32_t t = 0; t < n_terms; t++) {
				const void *col = (const void *)uni64((uint64_t)terms[first + t]);
				uint4 x[kDvPerThread];
#pragma unroll
				for (uint32_t q = 0; q < kDvPerThread; q++) x[q] = dv_gload(col, at[q]);
#pragma unroll
				for (uint32_t q = 0; q < kDvPerThread; q++) r[q] = uint4{r[q].x ^ x[q].x, r[q].y ^ x[q].y, r[q].z ^ x[q].z, r[q].w ^ x[q].w};
			}
			break;
		}
		}
#pragma unroll
		for (uint32_t q = 0; q < kDvPerThread; q++)
			if (j[q] < len) dv_gstore(out, j[q], r[q]);
	}
#undef DV_AT
}

hipError_t launch_derive_columns(hipStream_t s, const derive_job *d_jobs, uint32_t n_jobs, const void *const *d_terms, uint32_t total_units)
{
	if (n_jobs == 0 || total_units == 0) return hipSuccess;
	hipLaunchKernelGGL(k_derive_columns, dim3(total_units), dim3(256), 0, s, d_jobs, n_jobs, d_terms);
	return hipGetLastError();
}

} // namespace bn
