// binius_amd/csrc/kernels_flush.hip -- the masked flush witnesses of a batch of channel flushes (make_masked_flush_witnesses,
// core/src/constraint_system/prove.rs:671-881): for every flush f and row i below its selectors' common non-zero prefix
//   out_f[i] = (every selector bit is 1 at i) ? const_f + sum_j coeff_{f,j} * col_{f,j}[i] : ONE,
// the col_{f,j} subfield columns of tower level 0 or 3 .. 7 packed into F, the coefficients B128 (the mixing powers), the sum in
// B128.  Rows at and beyond the prefix are not written: the product tree counts them as ONE.
//
// k_flush_prefix: the non-zero prefix of every selector (count_zero_suffixes, prove.rs:883-902, at a 128-bit underlier): a workgroup
// scans a chunk of 16-byte elements and raises the selector's word to 128 * (1 + index of its last non-zero element).  The words stay
// in device memory; the main kernel takes the minimum over its flush's selectors itself.
//
// k_flush_witness: x -> coeff * x is GF(2)-linear, so the product with a level-l value is the XOR of 2^l / 4 nibble-table entries
// (ctable.hpp: T[p][e] = (e << 4p) * coeff, one table = one 256-byte LDS bank row, every ds_read_b128 conflict-free whatever the
// data).  A job is one flush, a unit (one workgroup) is a run of 2048 of its rows, eight per thread, found in the job table by
// bisection: one launch for every flush of the call.  The workgroup builds the tables of its flush in LDS -- 2, 4, 8, 16 or 32 per
// column of level 3 .. 7, none for a bit column (bit ? coeff : 0) or for a coefficient ONE (the value itself) -- and keeps the eight
// sums in registers.  Column values are loaded without a branch (rows beyond the prefix re-read a valid row and are not stored) and one
// column ahead of the lookups: with two workgroups per CU there are few waves to hide a load behind.  A flush with more than 256 tables (64 KiB) takes several passes over its columns: the tables are rebuilt, the
// sums stay where they are, so the output is still written once, with plain 16-byte stores.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "ctable.hpp"
#include "gf128.hpp"
#include "internal.hpp"

namespace bn {

namespace {

constexpr int kRowsPerThread = kFlushUnitRows / 256;
static_assert(kFlushUnitRows % 256 == 0 && kRowsPerThread == 8, "a thread owns rows r0 + tid + 256 k");

struct flush_smem {
	uint4 T[kFlushPassTables * 16]; // [table][entry]
	uint4 basis[128];               // coeff * 2^i of the column being built
};

// The rows of a thread are r0 + tid + 256 k; a row at or beyond `limit` reads row r0 instead (valid: r0 < limit) and is never stored,
// so neither the loads nor the lookups are under a branch: the eight loads of a column are in flight together.
__device__ __forceinline__ uint64_t fl_row(uint64_t r0, uint64_t limit, int k)
{
	const uint64_t row = r0 + threadIdx.x + 256u * k;
	return row < limit ? row : r0;
}

// the values of one column at the thread's eight rows (level 0: the bit)
template <int LEVEL>
__device__ __forceinline__ void fl_load(uint4 (&x)[kRowsPerThread], const void *__restrict__ col, uint64_t r0, uint64_t limit)
{
#pragma unroll
	for (int k = 0; k < kRowsPerThread; k++) {
		const uint64_t row = fl_row(r0, limit, k);
		if constexpr (LEVEL == 0) {
			x[k].x = (reinterpret_cast<const uint32_t *>(col)[row >> 5] >> (row & 31)) & 1u;
		} else if constexpr (LEVEL == 3) {
			x[k].x = reinterpret_cast<const uint8_t *>(col)[row];
		} else if constexpr (LEVEL == 4) {
			x[k].x = reinterpret_cast<const uint16_t *>(col)[row];
		} else if constexpr (LEVEL == 5) {
			x[k].x = reinterpret_cast<const uint32_t *>(col)[row];
		} else if constexpr (LEVEL == 6) {
			const uint2 v = reinterpret_cast<const uint2 *>(col)[row];
			x[k].x = v.x;
			x[k].y = v.y;
		} else {
			x[k] = reinterpret_cast<const uint4 *>(col)[row];
		}
	}
}

// ... into the eight sums.  tab == nullptr: the coefficient is ONE (levels >= 3); coeff: the coefficient of a level-0 column
template <int LEVEL>
__device__ __forceinline__ void fl_apply(uint4 (&acc)[kRowsPerThread], const uint4 (&x)[kRowsPerThread], const char *tab, uint4 coeff)
{
#pragma unroll
	for (int k = 0; k < kRowsPerThread; k++) {
		if constexpr (LEVEL == 0) {
			const uint32_t m = 0u - x[k].x;
			acc[k] = xor4(acc[k], uint4{coeff.x & m, coeff.y & m, coeff.z & m, coeff.w & m});
		} else if constexpr (LEVEL <= 5) {
			if (tab)
				ctable_lookup<(LEVEL == 3 ? 2 : LEVEL == 4 ? 4 : 8)>(acc[k], tab, x[k].x);
			else
				acc[k].x ^= x[k].x;
		} else if constexpr (LEVEL == 6) {
			if (tab) {
				ctable_lookup<8>(acc[k], tab, x[k].x);
				ctable_lookup<8>(acc[k], tab + 8 * 256, x[k].y);
			} else {
				acc[k].x ^= x[k].x;
				acc[k].y ^= x[k].y;
			}
		} else {
			if (tab) {
				ctable_lookup<8>(acc[k], tab, x[k].x);
				ctable_lookup<8>(acc[k], tab + 8 * 256, x[k].y);
				ctable_lookup<8>(acc[k], tab + 16 * 256, x[k].z);
				ctable_lookup<8>(acc[k], tab + 24 * 256, x[k].w);
			} else {
				acc[k] = xor4(acc[k], x[k]);
			}
		}
	}
}

__device__ __forceinline__ void fl_load_any(uint4 (&x)[kRowsPerThread], const flush_col *__restrict__ cols, uint32_t c, uint64_t r0, uint64_t limit)
{
	const void *col = (const void *)uni64((uint64_t)cols[c].ptr);
	switch (uni32(cols[c].level)) {
	case 0: fl_load<0>(x, col, r0, limit); break;
	case 3: fl_load<3>(x, col, r0, limit); break;
	case 4: fl_load<4>(x, col, r0, limit); break;
	case 5: fl_load<5>(x, col, r0, limit); break;
	case 6: fl_load<6>(x, col, r0, limit); break;
	default: fl_load<7>(x, col, r0, limit); break;
	}
}

} // namespace

// Workgroup w of selector s scans elements [c, c + kFlushSelChunk) of it, c = (w - start) * kFlushSelChunk.
__global__ __launch_bounds__(256) void k_flush_prefix(const flush_sel *__restrict__ sels, uint32_t n_sels)
{
	__shared__ unsigned long long best[4];
	const flush_sel &sl = sels[find_job(sels, n_sels, blockIdx.x)];
	const uint4 *col = (const uint4 *)uni64((uint64_t)sl.col);
	const uint64_t elems = uni64(sl.elems);
	const uint64_t c0 = (uint64_t)(blockIdx.x - uni32(sl.start)) * kFlushSelChunk;
	const uint64_t c1 = c0 + kFlushSelChunk < elems ? c0 + kFlushSelChunk : elems;
	unsigned long long last = 0; // 1 + index of the last non-zero element this thread saw
	for (uint64_t e = c0 + threadIdx.x; e < c1; e += 256) {
		const uint4 v = col[e];
		if (v.x | v.y | v.z | v.w) last = e + 1;
	}
	for (int d = 32; d >= 1; d >>= 1) {
		const unsigned long long o = __shfl_xor(last, d, 64);
		last = o > last ? o : last;
	}
	if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = last;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 4; w++) last = best[w] > last ? best[w] : last;
		if (last) atomicMax(reinterpret_cast<unsigned long long *>(sl.prefix), last * 128ull);
	}
}

// Unit u (one workgroup): rows [r0, r0 + 2048) of job j, r0 = (u - start) * 2048.
__global__ __launch_bounds__(256, 2) void k_flush_witness(const flush_job *__restrict__ jobs, uint32_t n_jobs)
{
	extern __shared__ uint4 fl_lds[];
	flush_smem &sm = *reinterpret_cast<flush_smem *>(fl_lds);
	const flush_job &jb = jobs[find_job(jobs, n_jobs, blockIdx.x)];
	const uint64_t rows = uni64(jb.rows);
	const uint32_t n_sels = uni32(jb.n_sels), n_passes = uni32(jb.n_passes);
	const flush_col *cols = (const flush_col *)uni64((uint64_t)jb.cols);
	const uint32_t *const *sels = (const uint32_t *const *)uni64((uint64_t)jb.sels);
	const uint64_t *sel_prefix = (const uint64_t *)uni64((uint64_t)jb.sel_prefix);
	uint4 *out = (uint4 *)uni64((uint64_t)jb.out);
	const uint64_t r0 = (uint64_t)(blockIdx.x - uni32(jb.start)) * kFlushUnitRows;
	uint64_t limit = rows;
	for (uint32_t s = 0; s < n_sels; s++) {
		const uint64_t p = uni64(sel_prefix[s]);
		limit = p < limit ? p : limit;
	}
	if (r0 >= limit) return; // (uniform: the whole unit lies in the tail that is not written)
	const uint4 c0 = to_u4(jb.const_term);
	uint4 acc[kRowsPerThread];
#pragma unroll
	for (int k = 0; k < kRowsPerThread; k++) acc[k] = c0;
#pragma unroll 1
	for (uint32_t p = 0; p < n_passes; p++) {
		const uint32_t first = uni32(jb.pass_first[p]), end = uni32(jb.pass_first[p + 1]);
		// (the first column's values travel while the tables are built)
		uint4 cur[kRowsPerThread], nxt[kRowsPerThread];
		fl_load_any(cur, cols, first, r0, limit);
		if (p) __syncthreads(); // (the readers of the previous pass's tables are done)
		// ---- the tables of this pass, column after column
#pragma unroll 1
		for (uint32_t c = first; c < end; c++) {
			const uint32_t table = uni32(cols[c].table);
			if (table == kFlushNoTable) continue;
			const uint32_t bits = 1u << uni32(cols[c].level), entries = bits << 2; // 2^l / 4 tables of 16 entries
			if (threadIdx.x < bits) sm.basis[threadIdx.x] = to_u4(mul_basis(cols[c].coeff, threadIdx.x));
			__syncthreads();
			for (uint32_t e = threadIdx.x; e < entries; e += 256) sm.T[table * 16 + e] = ctable_entry(sm.basis + ((e >> 4) << 2), e);
			__syncthreads(); // (the basis is rewritten by the next column; the tables are read below)
		}
		// ---- the columns of this pass into the sums: column c + 1 is loaded before column c is looked up
#pragma unroll 1
		for (uint32_t c = first; c < end; c++) {
			if (c + 1 < end) fl_load_any(nxt, cols, c + 1, r0, limit);
			const uint32_t table = uni32(cols[c].table);
			const char *tab = table == kFlushNoTable ? nullptr : reinterpret_cast<const char *>(sm.T) + (size_t)table * 256;
			switch (uni32(cols[c].level)) {
			case 0: fl_apply<0>(acc, cur, tab, to_u4(cols[c].coeff)); break;
			case 3: fl_apply<3>(acc, cur, tab, uint4{}); break;
			case 4: fl_apply<4>(acc, cur, tab, uint4{}); break;
			case 5: fl_apply<5>(acc, cur, tab, uint4{}); break;
			case 6: fl_apply<6>(acc, cur, tab, uint4{}); break;
			default: fl_apply<7>(acc, cur, tab, uint4{}); break;
			}
			if (c + 1 < end) {
#pragma unroll
				for (int k = 0; k < kRowsPerThread; k++) cur[k] = nxt[k];
			}
		}
	}
	// ---- the mask: a row at which some selector is off is ONE
	uint32_t on = (1u << kRowsPerThread) - 1;
#pragma unroll 1
	for (uint32_t s = 0; s < n_sels; s++) {
		const uint32_t *sel = (const uint32_t *)uni64((uint64_t)sels[s]);
		uint32_t w[kRowsPerThread];
#pragma unroll
		for (int k = 0; k < kRowsPerThread; k++) {
			const uint64_t row = fl_row(r0, limit, k);
			w[k] = (sel[row >> 5] >> (row & 31)) & 1u;
		}
#pragma unroll
		for (int k = 0; k < kRowsPerThread; k++) on &= ~((w[k] ^ 1u) << k);
	}
#pragma unroll
	for (int k = 0; k < kRowsPerThread; k++) {
		const uint64_t row = r0 + threadIdx.x + 256u * k;
		if (row < limit) out[row] = ((on >> k) & 1) ? acc[k] : uint4{1, 0, 0, 0};
	}
}

hipError_t launch_flush_prefix(hipStream_t s, const flush_sel *d_sels, uint32_t n_sels, uint32_t total_wgs)
{
	if (n_sels == 0 || total_wgs == 0) return hipSuccess;
	hipLaunchKernelGGL(k_flush_prefix, dim3(total_wgs), dim3(256), 0, s, d_sels, n_sels);
	return hipGetLastError();
}

hipError_t launch_flush_witness(hipStream_t s, const flush_job *d_jobs, uint32_t n_jobs, uint32_t total_units)
{
	if (n_jobs == 0 || total_units == 0) return hipSuccess;
	constexpr size_t lds = sizeof(flush_smem); // 66 KiB: two workgroups per CU
	const hipError_t attr = func_lds_limit(reinterpret_cast<const void *>(&k_flush_witness), (int)lds);
	if (attr != hipSuccess) return attr;
	hipLaunchKernelGGL(k_flush_witness, dim3(total_units), dim3(256), lds, s, d_jobs, n_jobs);
	return hipGetLastError();
}

} // namespace bn
