// binius_amd/csrc/kernels_merge.hip -- merge_multilins (crates/core/src/piop/prove.rs:78-118, P = F) for multilinears resident on the
// device: the FRI message of piop::commit in one launch.  With off_i the sum of the lengths of the multilinears after i,
//   message[r * 2^total_vars + off_i + bitrev(x, n_vars[i])] = multilins[i][x]      for every repeat r < 2^log_repeats,
// zeros from the end of the data to 2^total_vars in every repeat.  A batched bit-reversal permutation of 16-byte elements.
//
// Jobs (merge_job, sorted by first unit, found by bisection: batch.hpp) come in three forms:
//   tiled   L >= 2 T.  An index of L bits is hi[T] | mid[L - 2T] | lo[T], its reversal rev(lo) | rev(mid) | rev(hi).  A unit (one
//           workgroup) owns one mid value: it reads 2^T runs (one per hi) of 2^T contiguous elements, transposes them through LDS and
//           writes 2^T runs (one per rev(lo)) of 2^T contiguous elements, once per repeat: both sides of HBM see runs of 2^T * 16 bytes.
//           The LDS image is the OUTPUT tile, row rev(lo), column rev(hi): the permutation happens on the way in.  Eight neighbouring
//           lanes of the ds_write_b128 (one bank group: 128 bytes, eight 16-byte slots) hold eight consecutive lo, that is eight rows
//           whose top three bits differ, at one column -- one slot, eight-way.  Column c of row r is therefore kept at c ^ (r >> (T - 3)):
//           the eight lanes fall on eight slots.  The read side takes whole rows, a permutation of contiguous slots: conflict-free.
//   small   L < 2 T, down to L = 0: one unit per job, out[y] = src[rev(y)] read directly (at most 2^(2T - 1) elements).
//   zero    the tail of every repeat, units of kMergeZeroChunk elements.
// Plain 16-byte vector loads and stores, 64-bit element offsets throughout.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "internal.hpp"

namespace bn {

// A source pointer comes out of the job table, where the compiler sees a generic pointer: its loads would be flat loads, which may
// alias LDS and are then kept in order with the tile's writes, one wait per element.  Sources are device memory.
typedef uint32_t merge_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 merge_gload(const void *p, uint64_t idx)
{
	const merge_u32x4 x = ((const __attribute__((address_space(1))) merge_u32x4 *)(uintptr_t)p)[idx];
	return uint4{x.x, x.y, x.z, x.w};
}

template <int T>
__global__ __launch_bounds__(256) void k_merge_multilins(const merge_job *__restrict__ jobs, uint32_t n_jobs, uint4 *__restrict__ dst, uint32_t log_total,
                                                         uint32_t log_repeats)
{
	extern __shared__ uint4 mg_lds[];
	constexpr uint32_t S = 1u << T, Q = S * S / 256;
	const uint32_t tid = threadIdx.x, u = blockIdx.x;
	const merge_job &jb = jobs[find_job(jobs, n_jobs, u)];
	const uint4 *src = (const uint4 *)uni64((uint64_t)jb.src);
	const uint64_t off = uni64(jb.dst_off);
	const uint32_t L = uni32(jb.log_len), kind = uni32(jb.kind);
	const uint64_t rel = uni64(jb.first) + (u - uni32(jb.start)); // this unit within its job
	const uint64_t stride = (uint64_t)1 << log_total;
	const uint32_t reps = 1u << log_repeats;

	if (kind == kMergeTiled) {
		const uint32_t mid_bits = L - 2 * T, sh = L - T;
		const uint64_t rmid = mid_bits ? __brevll(rel) >> (64 - mid_bits) : 0;
		const uint4 *in = src + (rel << T);
		uint4 *out = dst + off + (rmid << T);
#pragma unroll
		for (uint32_t q = 0; q < Q; q++) {
			const uint32_t e = tid + 256 * q, h = e >> T, l = e & (S - 1);
			const uint32_t r = __brev(l) >> (32 - T), c = __brev(h) >> (32 - T);
			mg_lds[r * S + (c ^ (r >> (T - 3)))] = merge_gload(in, ((uint64_t)h << sh) + l);
		}
		__syncthreads();
		uint4 w[Q];
#pragma unroll
		for (uint32_t q = 0; q < Q; q++) {
			const uint32_t e = tid + 256 * q, r = e >> T, c = e & (S - 1);
			w[q] = mg_lds[r * S + (c ^ (r >> (T - 3)))];
		}
#pragma unroll 1
		for (uint32_t rep = 0; rep < reps; rep++) {
#pragma unroll
			for (uint32_t q = 0; q < Q; q++) {
				const uint32_t e = tid + 256 * q, r = e >> T, c = e & (S - 1);
				out[rep * stride + ((uint64_t)r << sh) + c] = w[q];
			}
		}
	} else if (kind == kMergeSmall) {
		const uint32_t len = 1u << L;
		for (uint32_t y = tid; y < len; y += 256) {
			const uint4 x = merge_gload(src, L ? __brev(y) >> (32 - L) : 0);
			for (uint32_t rep = 0; rep < reps; rep++) dst[rep * stride + off + y] = x;
		}
	} else {
		const uint64_t len = uni64(jb.len), base = rel * kMergeZeroChunk;
#pragma unroll 1
		for (uint32_t rep = 0; rep < reps; rep++) {
#pragma unroll
			for (uint32_t q = 0; q < kMergeZeroChunk / 256; q++) {
				const uint64_t i = base + tid + 256 * q;
				if (i < len) dst[rep * stride + off + i] = uint4{0, 0, 0, 0};
			}
		}
	}
}

hipError_t launch_merge_multilins(hipStream_t s, uint32_t t, const merge_job *d_jobs, uint32_t n_jobs, void *d_message, uint32_t log_total, uint32_t log_repeats,
                                  uint32_t total_units)
{
	if (n_jobs == 0 || total_units == 0) return hipSuccess;
	if (t != 5 && t != 6) return hipErrorInvalidValue;
	const size_t lds = (size_t)16 << (2 * t);
	const void *fn = t == 5 ? reinterpret_cast<const void *>(&k_merge_multilins<5>) : reinterpret_cast<const void *>(&k_merge_multilins<6>);
	const hipError_t attr = func_lds_limit(fn, (int)lds);
	if (attr != hipSuccess) return attr;
	if (t == 5)
		hipLaunchKernelGGL(k_merge_multilins<5>, dim3(total_units), dim3(256), lds, s, d_jobs, n_jobs, (uint4 *)d_message, log_total, log_repeats);
	else
		hipLaunchKernelGGL(k_merge_multilins<6>, dim3(total_units), dim3(256), lds, s, d_jobs, n_jobs, (uint4 *)d_message, log_total, log_repeats);
	return hipGetLastError();
}

} // namespace bn
