// binius_amd/csrc/kernels_fri_query.hip -- everything FRIFolder::finish_proof (crates/core/src/protocols/fri/prove.rs:483-507) writes
// to the decommitment, in one launch.  In 16-byte units (a field element; a digest is two), in transcript order:
//   header   terminate codeword | layer of oracle 0 | layer of oracle 1 | ...        (vcs_optimal_layers, prove.rs:597-610)
//   record q for oracle i:  2^log_coset_size values at (index_{q,i} << log_coset_size) of codeword i,
//                           then log_n_cosets - layer_depth digests, leaf sibling first (prove_coset_opening, prove.rs:613-637;
//                           BinaryMerkleTree::branch, merkle_tree/binary_merkle_tree.rs:121-141)
// with index_{q,i} = indices[q] >> shift_i.  Every piece is a copy: the work is addressing.
//
// Workgroups [0, header_wgs) copy the header, kFriQueryHeaderChunk units each: the terminate codeword and the layers are contiguous
// ranges of their sources.  Every later workgroup is four waves, one (query, oracle) opening per wave: lanes run over the units of the
// opening, so the coset is read coalesced (a wave loops when it has more than 64 units) and the branch is two units per level.  Level
// j of a tree of 2^L leaves starts at node (2^j - 1) << (L + 1 - j) of the flattened array (leaves first, root last), and the
// sibling of the opened path there is (index >> j) ^ 1.
//
// The launcher's caller (abi_fri_query.cpp) has checked every index against 2^index_bits and every shift and depth against the
// oracle's sizes: no address here leaves the arrays the descriptors name.  Plain 16-byte vector loads and stores, 64-bit offsets.
#include <hip/hip_runtime.h>

#include "internal.hpp"

namespace bn {

// (sources come out of the argument table as generic pointers; they are device memory: global loads, not flat ones)
typedef uint32_t fq_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 fq_gload(const void *p, uint64_t idx)
{
	const fq_u32x4 x = ((const __attribute__((address_space(1))) fq_u32x4 *)(uintptr_t)p)[idx];
	return uint4{x.x, x.y, x.z, x.w};
}

__global__ __launch_bounds__(256) void k_fri_query(const fri_query_args a, const uint64_t *__restrict__ indices, uint4 *__restrict__ out)
{
	const uint32_t tid = threadIdx.x;
	if (blockIdx.x < a.header_wgs) {
		const uint64_t base = (uint64_t)blockIdx.x * kFriQueryHeaderChunk;
#pragma unroll
		for (uint32_t k = 0; k < kFriQueryHeaderChunk / 256; k++) {
			const uint64_t u = base + tid + 256 * k;
			if (u >= a.header_elems) break;
			if (u < a.terminate_elems) {
				out[u] = fq_gload(a.terminate, u);
				continue;
			}
			// the layer that holds unit u: the last oracle whose layer starts at or before it
			uint32_t i = 0;
			while (i + 1 < a.n_oracles && a.o[i + 1].layer_off <= u) i++;
			const fri_query_oracle &o = a.o[i];
			// layer `depth` of the tree is digests [2^(L+1) - 2^(depth+1), 2^(L+1) - 2^depth) of the flattened array
			const uint64_t first = ((uint64_t)2 << o.log_n_cosets) - ((uint64_t)2 << o.layer_depth);
			out[u] = fq_gload(o.nodes, 2 * first + (u - o.layer_off));
		}
		return;
	}
	const uint32_t lane = tid & 63;
	const uint64_t w = (uint64_t)(blockIdx.x - a.header_wgs) * 4 + (tid >> 6);
	if (a.n_oracles == 0 || w >= (uint64_t)a.n_queries * a.n_oracles) return;
	const uint64_t q = w / a.n_oracles;
	const fri_query_oracle &o = a.o[w - q * a.n_oracles];
	const uint32_t L = o.log_n_cosets;
	const uint64_t index = indices[q] >> o.shift;
	const uint64_t n_vals = (uint64_t)1 << o.log_coset_size, n_units = n_vals + 2 * (uint64_t)(L - o.layer_depth);
	const uint64_t coset = index << o.log_coset_size;
	uint4 *dst = out + a.header_elems + q * a.record_elems + o.record_off;
	for (uint64_t u = lane; u < n_units; u += 64) {
		if (u < n_vals) {
			dst[u] = fq_gload(o.codeword, coset + u);
		} else {
			const uint32_t j = (uint32_t)((u - n_vals) >> 1);
			const uint64_t node = ((((uint64_t)1 << j) - 1) << (L + 1 - j)) | ((index >> j) ^ 1);
			dst[u] = fq_gload(o.nodes, 2 * node + ((u - n_vals) & 1));
		}
	}
}

hipError_t launch_fri_query(hipStream_t s, const fri_query_args &a, const uint64_t *d_indices, void *out)
{
	const uint64_t n_openings = (uint64_t)a.n_queries * a.n_oracles;
	const uint64_t blocks = a.header_wgs + (n_openings + 3) / 4;
	if (blocks == 0) return hipSuccess;
	if (blocks > (1u << 30)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_fri_query, dim3((unsigned)blocks), dim3(256), 0, s, a, d_indices, (uint4 *)out);
	return hipGetLastError();
}

} // namespace bn
