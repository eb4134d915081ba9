// binius_amd/csrc/pe_rows.hpp -- the row steps shared by the kernels that reduce a packed column over its high rows against a chunk
// of a tensor expansion staged in LDS (kernels_partial_eval.hip, kernels_mle_eval.hip): a 64-bit word of a bit column as the lane mask
// of 64 steps, and the subfield product of one packed value of level >= 3.
#pragma once
#include <hip/hip_runtime.h>

#include "ctable.hpp"
#include "gf128.hpp"
#include "internal.hpp"

namespace bn {

constexpr uint32_t kStageMask = (1u << kPeLogVecChunk) - 1;
// the 64-bit word lane k loaded, in a scalar register pair
__device__ __forceinline__ uint64_t lane_word(uint32_t w_lo, uint32_t w_hi, int k)
{
	return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)w_lo, k) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)w_hi, k) << 32);
}

// 64 steps of a wave: step k adds stage[index of k] under the mask that lane k loaded.  Eight LDS reads are issued before any is
// used; two steps are folded with one three-input XOR per word, each value selected under its mask (no branch).
// SMALL (b < 6): the index is ((s0 + k) << sh) + sub, passed as base | sh << 16, and is kept inside the stage (steps beyond a
// chunk of fewer than 64 words have mask 0); otherwise it is s0 + k < 1024, the same for every lane.
template <bool SMALL>
__device__ __forceinline__ void pe_block(uint4 &acc, uint32_t w_lo, uint32_t w_hi, const uint4 *stage, uint32_t packed)
{
	const uint32_t base = packed & 0xFFFFu, sh = packed >> 16;
#pragma unroll
	for (int k0 = 0; k0 < 64; k0 += 8) {
		uint4 v[8];
#pragma unroll
		for (int k = 0; k < 8; k++) v[k] = SMALL ? stage[(base + ((uint32_t)(k0 + k) << sh)) & kStageMask] : stage[k0 + k];
		__builtin_amdgcn_sched_barrier(0);
#pragma unroll
		for (int k = 0; k < 8; k += 2) {
			const bool on0 = __builtin_amdgcn_inverse_ballot_w64(lane_word(w_lo, w_hi, k0 + k)), on1 = __builtin_amdgcn_inverse_ballot_w64(lane_word(w_lo, w_hi, k0 + k + 1));
			acc.x = ct_xor3(acc.x, on0 ? v[k].x : 0u, on1 ? v[k + 1].x : 0u);
			acc.y = ct_xor3(acc.y, on0 ? v[k].y : 0u, on1 ? v[k + 1].y : 0u);
			acc.z = ct_xor3(acc.z, on0 ? v[k].z : 0u, on1 ? v[k + 1].z : 0u);
			acc.w = ct_xor3(acc.w, on0 ? v[k].w : 0u, on1 ? v[k + 1].w : 0u);
		}
	}
}

// x * (value idx of a column packed at tower level IOTA >= 3)
template <int IOTA>
__device__ __forceinline__ f128 pe_mul(f128 x, const uint64_t *__restrict__ words, uint64_t idx)
{
	if constexpr (IOTA == 7) {
		return mul_slow(x, f128{words[2 * idx], words[2 * idx + 1]});
	} else if constexpr (IOTA == 6) {
		return mul_walk<6>(x, words[idx]);
	} else {
		constexpr unsigned W = 1u << IOTA, PER = 64 / W;
		return mul_walk<IOTA>(x, (words[idx / PER] >> ((idx % PER) * W)) & ((1ull << W) - 1));
	}
}

} // namespace bn
