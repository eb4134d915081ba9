// binius_amd/csrc/kernels_compose_tower.hip -- bn_compute_composite with a tower-typed expression (bn_expr_compile_tower): a computed
// column of a constraint system at its own tower level from the columns it is a function of, each at ITS level (m3's add_computed:
// m3/src/builder/constraint_system.rs:515-540 -- the LinearCombination and Composite variants of MultilinearPolyVariant,
// multilinear.rs of core's oracle module; value by value: constraint_system/validate.rs:151-279).
//
// A streaming kernel in the frame of kernels_derive.hip: a workgroup takes kComposeUnitElems contiguous 16-byte OUTPUT elements, a
// chunk of 256 Q at a time, thread t the elements t, t + 256, ... of the chunk, so every store of a wave is one run of 1 KiB.  The
// program (compose_tower.hpp) is interpreted once per chunk on Q elements per thread: an operand that is an input issues its Q loads
// before any of them is used.  The 2^(7 - L) values of an output element that an input of level l <= L holds are one aligned piece
// of 2^(7 - L + l) bits of ONE input element (neighbouring threads share it); ct_spread moves them to their places.  Intermediate
// values live in LDS as [slot][q][word][thread] -- a thread reads only what it wrote, so there is no barrier --, sized by the
// expression's live count: Q = 4, 2 or 1 elements per thread for up to 4, 8 or 16 slots (64 KiB at most).  Indices of elements past
// the end are clamped to the last element and only the store is predicated.  Every loop bound comes from the program or the levels,
// never from the data; 64-bit element offsets throughout.
#include <hip/hip_runtime.h>

#include "compose_tower.hpp"
#include "internal.hpp"

namespace bn {

typedef uint32_t compose_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f128 ct_gload(const void *p, uint64_t idx)
{
	const compose_u32x4 x = ((const __attribute__((address_space(1))) compose_u32x4 *)(uintptr_t)p)[idx];
	return f128{(uint64_t)x.x | ((uint64_t)x.y << 32), (uint64_t)x.z | ((uint64_t)x.w << 32)};
}
__device__ __forceinline__ void ct_gstore(void *p, uint64_t idx, f128 v)
{
	((__attribute__((address_space(1))) compose_u32x4 *)(uintptr_t)p)[idx] =
		compose_u32x4{(uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32)};
}

template <uint32_t Q>
struct ct_frame {
	uint32_t *lds;
	uint32_t tid;
	const void *const *rows;
	const f128 *consts;
	const uint32_t *in_levels;
	uint32_t L;
	uint64_t at[Q]; // the (clamped) output element of each of the thread's Q values

	__device__ __forceinline__ uint32_t word(uint32_t slot, uint32_t q, uint32_t w) const { return ((slot * Q + q) * 4 + w) * 256 + tid; }
	__device__ __forceinline__ void fetch(uint32_t operand, f128 (&v)[Q]) const
	{
		const uint32_t idx = operand & kCtIdxMask;
		switch (operand & kCtTagMask) {
		case kCtSlot:
#pragma unroll
			for (uint32_t q = 0; q < Q; q++)
				v[q] = f128{(uint64_t)lds[word(idx, q, 0)] | ((uint64_t)lds[word(idx, q, 1)] << 32), (uint64_t)lds[word(idx, q, 2)] | ((uint64_t)lds[word(idx, q, 3)] << 32)};
			break;
		case kCtInput: {
			const void *col = rows[idx];
			const uint32_t l = in_levels[idx], d = L - l;
#pragma unroll
			for (uint32_t q = 0; q < Q; q++) v[q] = ct_gload(col, at[q] >> d);
			if (d) {
#pragma unroll
				for (uint32_t q = 0; q < Q; q++) v[q] = ct_spread(v[q], at[q], l, L);
			}
			break;
		}
		default: {
			const f128 c = consts[idx];
#pragma unroll
			for (uint32_t q = 0; q < Q; q++) v[q] = c;
			break;
		}
		}
	}
	__device__ __forceinline__ void put(uint32_t slot, const f128 (&v)[Q]) const
	{
#pragma unroll
		for (uint32_t q = 0; q < Q; q++) {
			lds[word(slot, q, 0)] = (uint32_t)v[q].lo;
			lds[word(slot, q, 1)] = (uint32_t)(v[q].lo >> 32);
			lds[word(slot, q, 2)] = (uint32_t)v[q].hi;
			lds[word(slot, q, 3)] = (uint32_t)(v[q].hi >> 32);
		}
	}
};

template <uint32_t Q>
__global__ __launch_bounds__(256) void k_compose_tower(compose_tower_args A)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t ct_lds[];
	ct_frame<Q> F;
	F.lds = ct_lds;
	F.tid = threadIdx.x;
	F.rows = A.rows;
	F.consts = (const f128 *)A.consts;
	F.in_levels = A.in_levels;
	F.L = A.out_level;
	const ct_op *ops = (const ct_op *)A.ops;
	const uint64_t len = A.out_elems;
	const uint64_t unit_first = (uint64_t)blockIdx.x * kComposeUnitElems;
	constexpr uint32_t kChunk = 256 * Q;
#pragma unroll 1
	for (uint32_t c = 0; c < kComposeUnitElems / kChunk; c++) {
		const uint64_t first = unit_first + (uint64_t)c * kChunk;
		if (first >= len) break;
		uint64_t j[Q];
#pragma unroll
		for (uint32_t q = 0; q < Q; q++) {
			j[q] = first + F.tid + 256 * q;
			F.at[q] = j[q] < len ? j[q] : len - 1;
		}
#pragma unroll 1
		for (uint32_t i = 0; i < A.n_ops; i++) {
			const ct_op op = ops[i];
			f128 a[Q], b[Q];
			F.fetch(op.a, a);
			if (op.kind == BN_STEP_ADD) {
				F.fetch(op.b, b);
#pragma unroll
				for (uint32_t q = 0; q < Q; q++) a[q] ^= b[q];
			} else if (op.kind == BN_STEP_MUL) {
				F.fetch(op.b, b);
#pragma unroll
				for (uint32_t q = 0; q < Q; q++) a[q] = ct_mul(a[q], b[q], op.level, F.L);
			} else {
#pragma unroll
				for (uint32_t q = 0; q < Q; q++) a[q] = ct_pow(a[q], op.exp, op.level, F.L);
			}
			F.put(op.dst, a);
		}
		f128 r[Q];
		F.fetch(A.result, r);
#pragma unroll
		for (uint32_t q = 0; q < Q; q++)
			if (j[q] < len) ct_gstore(A.out, j[q], r[q]);
	}
}

uint32_t compose_tower_per_thread(uint32_t n_slots) { return n_slots <= 4 ? 4 : n_slots <= 8 ? 2 : 1; }

hipError_t launch_compose_tower(hipStream_t s, const compose_tower_args &a, uint32_t n_slots)
{
	if (a.out_elems == 0) return hipSuccess;
	if (n_slots > BN_TOWER_EXPR_MAX_LIVE) return hipErrorInvalidValue;
	const uint64_t units = (a.out_elems + kComposeUnitElems - 1) / kComposeUnitElems;
	if (units > 0x7fffffffull) return hipErrorInvalidValue;
	const uint32_t q = compose_tower_per_thread(n_slots);
	const size_t lds = (size_t)(n_slots ? n_slots : 1) * q * 16 * 256; // <= 64 KiB
	if (q == 4)
		hipLaunchKernelGGL(k_compose_tower<4>, dim3((uint32_t)units), dim3(256), lds, s, a);
	else if (q == 2)
		hipLaunchKernelGGL(k_compose_tower<2>, dim3((uint32_t)units), dim3(256), lds, s, a);
	else
		hipLaunchKernelGGL(k_compose_tower<1>, dim3((uint32_t)units), dim3(256), lds, s, a);
	return hipGetLastError();
}

} // namespace bn
