// binius_amd/csrc/groupmul.hpp -- a GF(2^128) product computed by a group of G lanes (kernels_pairtree.hip, kernels_prodtree.hip):
// lane j multiplies b by the j-th (128 / G)-bit limb of a, moves the partial product to its place, and the G partial products
// are XORed across the lanes (DPP inside a row of 16, bpermute above).
#pragma once
#include <hip/hip_runtime.h>

#include "gf128.hpp"

namespace bn {
namespace {

template <int K>
__device__ __forceinline__ f128 place_limb(f128 r, unsigned j)
{
	// r * 2^(j * 2^K): X_k for every bit k - K of j
	if constexpr (K <= 0) { if (j & (1u << (0 - K))) r = mulx<0>(r); }
	if constexpr (K <= 1) { if (j & (1u << (1 - K))) r = mulx<1>(r); }
	if constexpr (K <= 2) { if (j & (1u << (2 - K))) r = mulx<2>(r); }
	if constexpr (K <= 3) { if (j & (1u << (3 - K))) r = mulx<3>(r); }
	if constexpr (K <= 4) { if (j & (1u << (4 - K))) r = mulx<4>(r); }
	if constexpr (K <= 5) { if (j & (1u << (5 - K))) r = mulx<5>(r); }
	if constexpr (K <= 6) { if (j & (1u << (6 - K))) r = mulx<6>(r); }
	return r;
}

template <int CTRL>
__device__ __forceinline__ uint32_t xor_dpp(uint32_t x) { return x ^ (uint32_t)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xF, 0xF, true); }

// XOR over the G lanes of a group (G a power of two, groups aligned); every lane ends up with the sum
template <int G>
__device__ __forceinline__ uint32_t group_xor(uint32_t x)
{
	if constexpr (G >= 2) x = xor_dpp<0xB1>(x);  // quad_perm [1,0,3,2]
	if constexpr (G >= 4) x = xor_dpp<0x4E>(x);  // quad_perm [2,3,0,1]
	if constexpr (G >= 8) x = xor_dpp<0x141>(x); // row_half_mirror: lane 7 - j (the other quad)
	if constexpr (G >= 16) x = xor_dpp<0x140>(x); // row_mirror: lane 15 - j (the other half row)
	if constexpr (G >= 32) x ^= (uint32_t)__shfl_xor((int)x, 16);
	if constexpr (G >= 64) x ^= (uint32_t)__shfl_xor((int)x, 32);
	return x;
}

// a * b by the G lanes of a group; j = this lane's index in the group; the product is valid in every lane
template <int G>
__device__ __forceinline__ f128 group_product(f128 a, f128 b, unsigned j)
{
	constexpr int K = G == 8 ? 4 : (G == 16 ? 3 : (G == 32 ? 2 : 1));
	constexpr unsigned W = 1u << K;
	const unsigned bit = j * W;
	const uint64_t word = (bit & 64) ? a.hi : a.lo;
	const uint64_t limb = (word >> (bit & 63)) & ((1ull << W) - 1);
	f128 r = mul_walk<K>(b, limb);
	r = place_limb<K>(r, j);
	uint32_t w0 = group_xor<G>((uint32_t)r.lo), w1 = group_xor<G>((uint32_t)(r.lo >> 32));
	uint32_t w2 = group_xor<G>((uint32_t)r.hi), w3 = group_xor<G>((uint32_t)(r.hi >> 32));
	return f128{(uint64_t)w0 | ((uint64_t)w1 << 32), (uint64_t)w2 | ((uint64_t)w3 << 32)};
}

} // namespace
} // namespace bn
