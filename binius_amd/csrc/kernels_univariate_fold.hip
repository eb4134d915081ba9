// binius_amd/csrc/kernels_univariate_fold.hip -- the fold of the univariate round of the univariate-skip zerocheck for a batch of columns
// (ZerocheckProverImpl::fold_univariate_round, core/src/protocols/sumcheck/prove/zerocheck.rs:384-434: evaluate_partial_low at a query
// whose expansion is the Lagrange coefficients): for every column c of n_c variables and x < 2^(n_c - k)
//   out_c[x] = sum_{u < 2^k} coeffs[u] * M_c(u + 2^k x),
// M_c a column of tower level 0 (B1) or 3 (B8) packed into F, the 2^k coefficients in B128 and THE SAME for every column.
//
// The 2^k values of one output are a ROW of the column: 2^k bits at level 0, 2^k bytes at level 3, contiguous.  m -> coeffs[u] * m is
// GF(2)-linear, so the output is the XOR over the nibbles of the row of one nibble-table entry each (ctable.hpp: one table = 16 entries =
// one 256-byte LDS bank row, every ds_read_b128 conflict-free whatever the data):
//   level 0:  table p covers the bits u = 4p .. 4p + 3 of the row:   T[p][e]      = XOR_{b in e} coeffs[4p + b]
//   level 3:  tables 2u, 2u + 1 cover the two nibbles of byte u:      T[2u + h][e] = coeffs[u] * (e << 4h) = XOR_{b in e} coeffs[u] * 2^(4h + b)
// In both layouts nibble p of the row reads table p, so the streaming code depends only on the width of a row.  2^k / 4 tables at
// level 0 (16 KiB at k = 8), 2^(k + 1) at level 3: 64 KiB at k = 7; at k = 8 the 128 KiB are taken in two passes over u of 64 KiB
// each, the partial sums of a unit stay in registers between them and the output is written once.
//
// A job is one column, a unit a run of 2048 outputs of it (512 for rows of 64 bytes and more), eight (two) per thread, thread t of the
// workgroup owning the outputs r0 + t + 256 j: the 16-byte stores of a wave are contiguous.  The jobs are sorted by level and workgroup
// w takes the contiguous units [w U / W, (w + 1) U / W) of the launch: it builds the tables of a level once and streams all its units
// of that level through them (only level 3 at k = 8 rebuilds, per unit and pass).  Rows of 16 bytes and more are loaded as 16-byte
// vectors, all of a batch of rows (32 registers) before the first lookup; a narrower row is the lane's own word of a 16-byte element
// that 2 .. 64 neighbouring lanes share, so the wave's request is still one contiguous run.  A row beyond the column's end re-reads the
// unit's first row and is not stored: neither loads nor lookups are under a branch.  ONE launch for every column, size and level of a call.
// The kernel is instantiated per k (its two row widths: 2^k bits and 2^k bytes): with all eleven widths behind one switch the compiler
// kept the address arithmetic of every case live and spilled.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "ctable.hpp"
#include "gf128.hpp"
#include "internal.hpp"

namespace bn {

namespace {

// After every ctable_lookup: pins the schedule.  Left alone, the scheduler hoists the lookups of all the rows of a batch to the front and spills.
__device__ __forceinline__ void uf_pin(uint4 &acc) { asm volatile("" : "+v"(acc.x), "+v"(acc.y), "+v"(acc.z), "+v"(acc.w)::"memory"); }

// The part of row x that one pass covers: B bits (B < 32: in the low bits of w[0]).  ROW_U4: 16-byte vectors of a whole row (B >= 128),
// first_u4: where the pass begins inside the row.
template <int B, int ROW_U4>
__device__ __forceinline__ void uf_load(uint32_t (&w)[B >= 32 ? B / 32 : 1], const void *__restrict__ col, uint64_t x, uint32_t first_u4)
{
	if constexpr (B < 32) {
		const uint64_t bit = x * B;
		w[0] = (reinterpret_cast<const uint32_t *>(col)[bit >> 5] >> (bit & 31)) & ((1u << B) - 1u);
	} else if constexpr (B == 32) {
		w[0] = reinterpret_cast<const uint32_t *>(col)[x];
	} else if constexpr (B == 64) {
		const uint2 v = reinterpret_cast<const uint2 *>(col)[x];
		w[0] = v.x;
		w[1] = v.y;
	} else {
		const uint4 *p = reinterpret_cast<const uint4 *>(col) + x * ROW_U4 + first_u4;
#pragma unroll
		for (int u = 0; u < B / 128; u++) {
			const uint4 v = p[u];
			w[4 * u] = v.x;
			w[4 * u + 1] = v.y;
			w[4 * u + 2] = v.z;
			w[4 * u + 3] = v.w;
		}
	}
}

// One pass of one unit: the thread's RT rows r0 + tid + 256 j into acc[j], in batches of rows whose loads (at most eight 16-byte
// vectors) are all issued before the first lookup.
template <int B, int ROW_U4, int RT>
__device__ __forceinline__ void uf_rows(uint4 (&acc)[8], const char *__restrict__ T, const void *__restrict__ col, uint64_t r0, uint64_t out_len,
                                        uint32_t first_u4)
{
	constexpr int NW = B >= 32 ? B / 32 : 1;
	constexpr int R = B >= 1024 ? 1 : B >= 512 ? 2 : B >= 256 ? 4 : 8; // rows of a batch
	static_assert(RT % R == 0 && RT <= 8, "whole batches");
#pragma unroll
	for (int j0 = 0; j0 < RT; j0 += R) {
		uint32_t w[R][NW];
#pragma unroll
		for (int r = 0; r < R; r++) {
			const uint64_t row = r0 + threadIdx.x + 256u * (j0 + r);
			uf_load<B, ROW_U4>(w[r], col, row < out_len ? row : r0, first_u4);
		}
#pragma unroll
		for (int r = 0; r < R; r++) {
			if constexpr (B < 32) {
				ctable_lookup<(B <= 4 ? 1 : B / 4)>(acc[j0 + r], T, w[r][0]);
				uf_pin(acc[j0 + r]);
			} else {
#pragma unroll
				for (int q = 0; q < NW; q++) {
					ctable_lookup<8>(acc[j0 + r], T + q * 8 * 256, w[r][q]);
					uf_pin(acc[j0 + r]);
				}
			}
		}
	}
}

// The tables of (level, pass) into T.  First the entries 1, 2, 4, 8 of every table (the basis products), then the other twelve as their
// XORs.  Begins and ends with a workgroup barrier.
__device__ __forceinline__ void uf_build(uint4 *__restrict__ T, const uint4 *__restrict__ coeffs, uint32_t level, uint32_t k, uint32_t pass)
{
	const uint32_t n_tables = uf_tables(level, k);
	__syncthreads(); // (the readers of the previous tables are done)
	for (uint32_t i = threadIdx.x; i < n_tables * 4; i += 256) {
		const uint32_t t = i >> 2, b = i & 3;
		uint4 v{0, 0, 0, 0};
		if (level == 0) {
			const uint32_t u = 4 * t + b;
			if (u < (1u << k)) v = coeffs[u];
		} else {
			const uint32_t u = pass * (kUfPassTables / 2) + (t >> 1);
			v = to_u4(mul_basis(to_f128(coeffs[u]), 4 * (t & 1) + b));
		}
		T[t * 16 + (1u << b)] = v;
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < n_tables * 16; i += 256) {
		const uint32_t e = i & 15;
		if (e && !(e & (e - 1))) continue; // (a basis entry)
		T[i] = ctable_entry<true>(T + (i & ~15u), e);
	}
	__syncthreads();
}

} // namespace

// B, ROW_U4, RT of uf_rows for rows of 2^LRB bits
template <int LRB>
__device__ __forceinline__ void uf_pass(uint4 (&acc)[8], const char *__restrict__ T, const void *__restrict__ col, uint64_t r0, uint64_t out_len, uint32_t pass)
{
	constexpr int B = LRB > 10 ? 1024 : 1 << LRB;
	constexpr int ROW_U4 = LRB >= 7 ? 1 << (LRB - 7) : 1;
	uf_rows<B, ROW_U4, (int)uf_rows_per_thread(LRB)>(acc, T, col, r0, out_len, LRB > 10 ? 8 * pass : 0);
}

// One instantiation per skip_rounds K: its rows are 2^K bits (level 0) or 2^(K + 3) bits (level 3) wide.
template <int K>
__global__ __launch_bounds__(256, 2) void k_univariate_fold(const uf_job *__restrict__ jobs, uint32_t n_jobs, const uint4 *__restrict__ coeffs, uint32_t total_units)
{
	extern __shared__ uint4 uf_T[];
	const char *T = reinterpret_cast<const char *>(uf_T);
	const uint32_t u_begin = (uint32_t)((uint64_t)blockIdx.x * total_units / gridDim.x);
	const uint32_t u_end = (uint32_t)((uint64_t)(blockIdx.x + 1) * total_units / gridDim.x);
	if (u_begin >= u_end) return;
	uint32_t j = find_job(jobs, n_jobs, u_begin);
	uint32_t built = ~0u; // 2 * level + pass of the tables in LDS
#pragma unroll 1
	for (uint32_t u = u_begin; u < u_end; u++) {
		while (j + 1 < n_jobs && uni32(jobs[j + 1].start) <= u) j++;
		const uf_job &jb = jobs[j];
		const void *col = (const void *)uni64((uint64_t)jb.col);
		uint4 *out = (uint4 *)uni64((uint64_t)jb.out);
		const uint64_t out_len = uni64(jb.out_len);
		const uint32_t level = uni32(jb.level);
		const uint32_t rt = uf_rows_per_thread(K + level);
		const uint64_t r0 = (uint64_t)(u - uni32(jb.start)) * (256u * rt);
		const uint32_t n_passes = K + level > 10 ? 2 : 1;
		uint4 acc[8];
#pragma unroll
		for (int q = 0; q < 8; q++) acc[q] = uint4{0, 0, 0, 0};
#pragma unroll 1
		for (uint32_t p = 0; p < n_passes; p++) {
			if (built != 2 * level + p) {
				uf_build(uf_T, coeffs, level, K, p);
				built = 2 * level + p;
			}
			if (level == 0)
				uf_pass<K>(acc, T, col, r0, out_len, p);
			else
				uf_pass<K + 3>(acc, T, col, r0, out_len, p);
		}
#pragma unroll
		for (int q = 0; q < 8; q++) {
			const uint64_t row = r0 + threadIdx.x + 256u * q;
			if ((uint32_t)q < rt && row < out_len) out[row] = acc[q];
		}
	}
}

template <int K>
static hipError_t run_univariate_fold(hipStream_t s, const uf_job *d_jobs, uint32_t n_jobs, const void *d_coeffs, uint32_t total_units, uint32_t n_wgs, size_t lds)
{
	const hipError_t attr = func_lds_limit(reinterpret_cast<const void *>(&k_univariate_fold<K>), (int)lds);
	if (attr != hipSuccess) return attr;
	hipLaunchKernelGGL(k_univariate_fold<K>, dim3(n_wgs), dim3(256), lds, s, d_jobs, n_jobs, (const uint4 *)d_coeffs, total_units);
	return hipGetLastError();
}

hipError_t launch_univariate_fold(hipStream_t s, const uf_job *d_jobs, uint32_t n_jobs, const void *d_coeffs, uint32_t k, uint32_t total_units,
                                  uint32_t n_wgs, uint32_t lds_tables)
{
	if (n_jobs == 0 || total_units == 0 || n_wgs == 0) return hipSuccess;
	const size_t lds = (size_t)lds_tables * 256;
	switch (k) {
	case 1: return run_univariate_fold<1>(s, d_jobs, n_jobs, d_coeffs, total_units, n_wgs, lds);
	case 2: return run_univariate_fold<2>(s, d_jobs, n_jobs, d_coeffs, total_units, n_wgs, lds);
	case 3: return run_univariate_fold<3>(s, d_jobs, n_jobs, d_coeffs, total_units, n_wgs, lds);
	case 4: return run_univariate_fold<4>(s, d_jobs, n_jobs, d_coeffs, total_units, n_wgs, lds);
	case 5: return run_univariate_fold<5>(s, d_jobs, n_jobs, d_coeffs, total_units, n_wgs, lds);
	case 6: return run_univariate_fold<6>(s, d_jobs, n_jobs, d_coeffs, total_units, n_wgs, lds);
	case 7: return run_univariate_fold<7>(s, d_jobs, n_jobs, d_coeffs, total_units, n_wgs, lds);
	case 8: return run_univariate_fold<8>(s, d_jobs, n_jobs, d_coeffs, total_units, n_wgs, lds);
	default: return hipErrorInvalidValue;
	}
}

} // namespace bn
