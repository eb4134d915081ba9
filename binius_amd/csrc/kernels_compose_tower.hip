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
//
// k_compose_tower_batch serves a TABLE of such jobs in one launch (bn_expr_compile_tower_batch, compose_batch.hpp): the grid is the
// jobs' units one after the other, a workgroup finds its job by bisection (batch.hpp) and runs the same chunk loop on the job's
// program, rows and output range.
#include <hip/hip_runtime.h>

#include "batch.hpp"
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

// One unit -- kComposeUnitElems output elements from `unit_first` on -- of the program `ops[0 .. n_ops)` at Q elements per thread: the
// chunk loop of both kernels.  `len` is the column's (the job's) element count: indices past it are clamped for the loads, and only
// the store is predicated.
template <uint32_t Q>
__device__ __forceinline__ void ct_run_unit(uint32_t *lds, const void *const *rows, const f128 *consts, const uint32_t *in_levels, const ct_op *ops, uint32_t n_ops,
                                            uint32_t result, uint32_t L, uint64_t len, void *out, uint64_t unit_first)
{
	ct_frame<Q> F;
	F.lds = lds;
	F.tid = threadIdx.x;
	F.rows = rows;
	F.consts = consts;
	F.in_levels = in_levels;
	F.L = L;
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
		for (uint32_t i = 0; i < n_ops; i++) {
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
		F.fetch(result, r);
#pragma unroll
		for (uint32_t q = 0; q < Q; q++)
			if (j[q] < len) ct_gstore(out, j[q], r[q]);
	}
}

template <uint32_t Q>
__global__ __launch_bounds__(256) void k_compose_tower(compose_tower_args A)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t ct_lds[];
	ct_run_unit<Q>(ct_lds, A.rows, (const f128 *)A.consts, A.in_levels, (const ct_op *)A.ops, A.n_ops, A.result, A.out_level, A.out_elems, A.out,
	               (uint64_t)blockIdx.x * kComposeUnitElems);
}

// A batch (compose_batch.hpp): workgroup u serves unit u - start of the job that owns it.  The job's fields are the same in every lane
// and go to scalar registers; the branch on its class is workgroup-uniform.  The LDS of the launch is the largest job's: a job of a
// smaller class indexes [slot][q][word][thread] with its own Q inside it.
__global__ __launch_bounds__(256) void k_compose_tower_batch(compose_batch_args A)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t ct_lds[];
	const uint32_t unit = blockIdx.x;
	const compose_batch_job *job = A.jobs + uni32(find_job(A.jobs, A.n_jobs, unit));
	const uint32_t q = uni32(job->q), n_ops = uni32(job->n_ops), result = uni32(job->result), L = uni32(job->out_level);
	const uint64_t len = uni64(job->out_elems);
	const uint64_t unit_first = (uint64_t)(unit - uni32(job->start)) * kComposeUnitElems;
	const ct_op *ops = (const ct_op *)A.ops + uni32(job->ops_off);
	const f128 *consts = (const f128 *)A.consts + uni32(job->consts_off);
	const uint32_t *in_levels = A.in_levels + uni32(job->levels_off);
	const void *const *rows = A.rows + uni32(job->first_row);
	void *out = (char *)A.out + 16 * uni64(job->out_offset);
	if (q == 4)
		ct_run_unit<4>(ct_lds, rows, consts, in_levels, ops, n_ops, result, L, len, out, unit_first);
	else if (q == 2)
		ct_run_unit<2>(ct_lds, rows, consts, in_levels, ops, n_ops, result, L, len, out, unit_first);
	else
		ct_run_unit<1>(ct_lds, rows, consts, in_levels, ops, n_ops, result, L, len, out, unit_first);
}

hipError_t launch_compose_tower(hipStream_t s, const compose_tower_args &a, uint32_t n_slots)
{
	if (a.out_elems == 0) return hipSuccess;
	if (n_slots > BN_TOWER_EXPR_MAX_LIVE) return hipErrorInvalidValue;
	const uint64_t units = (a.out_elems + kComposeUnitElems - 1) / kComposeUnitElems;
	if (units > 0x7fffffffull) return hipErrorInvalidValue;
	const uint32_t q = compose_tower_per_thread(n_slots);
	const size_t lds = compose_tower_lds_bytes(n_slots); // <= 64 KiB
	if (q == 4)
		hipLaunchKernelGGL(k_compose_tower<4>, dim3((uint32_t)units), dim3(256), lds, s, a);
	else if (q == 2)
		hipLaunchKernelGGL(k_compose_tower<2>, dim3((uint32_t)units), dim3(256), lds, s, a);
	else
		hipLaunchKernelGGL(k_compose_tower<1>, dim3((uint32_t)units), dim3(256), lds, s, a);
	return hipGetLastError();
}

hipError_t launch_compose_tower_batch(hipStream_t s, const compose_batch_args &a, uint32_t total_units, uint32_t lds_bytes)
{
	if (total_units == 0 || a.n_jobs == 0) return hipSuccess;
	if (total_units > 0x7fffffffu || lds_bytes > (64u << 10)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_compose_tower_batch, dim3(total_units), dim3(256), lds_bytes, s, a);
	return hipGetLastError();
}

} // namespace bn
