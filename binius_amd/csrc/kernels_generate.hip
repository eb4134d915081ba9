// binius_amd/csrc/kernels_generate.hip -- the columns of a constraint system that a few integers, one field element or a 0/1 projection
// of a column on the device determine, written there at their own tower level: Projected at a hypercube vertex (add_selected /
// add_projected of m3: math/src/multilinear_extension.rs:193-237, constraint_system/validate.rs:239-254), Constant, StepDown, StepUp,
// SelectRow and Powers (core/src/transparent/), the incrementing column (m3/src/builder/structured.rs:64-81).  Every job of a call in ONE
// launch.
//
// The frame is kernels_derive.hip's: the host (abi_generate.cpp) turns every job into one of eight FORMS whose parameters are in bit
// coordinates (internal.hpp, generate_job), jobs are sorted by first unit and found by bisection (batch.hpp), a unit (one workgroup)
// is a run of contiguous 16-byte outputs of one job (4096, or 1024 where an output element is made of several input elements or of field products), taken in chunks of 1024, thread t owning elements t, t + 256, ... of a
// chunk.  A projection reads the inner column with plain 16-byte loads: whole elements when a run is at least one element
// (kGnProjElem); otherwise an output element is put together from pieces, one piece per input element, the loads of two pieces of each
// of the thread's four elements issued before any is used (kGnProjField: one run per input element; kGnProjSpread: the runs of an input
// element pushed together by a logarithmic compress).  Indices of elements past the job's end are clamped to its last element and only
// the store is predicated.  The fills are functions of the element's index and load nothing.  Powers: the host passes base^(2^b); a
// thread multiplies the entries of the set bits of its first value's index, then steps by the entries of its strides (1 inside an
// element, 256 elements between its elements), with gf128.hpp's product of the level.  64-bit element offsets throughout.
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "internal.hpp"

namespace bn {

constexpr uint32_t kGnPerThread = 4;                              // elements a thread holds at a time
constexpr uint32_t kGnChunkElems = 256 * kGnPerThread;            // elements the workgroup handles at a time
static_assert(kGenerateUnitElems % kGnChunkElems == 0 && kGeneratePieceUnitElems % kGnChunkElems == 0 && kGeneratePieceUnitElems > 0, "a unit is whole chunks of 1024 elements");

// (a pointer out of the job table is a generic pointer to the compiler: say that it is device memory, for global instead of flat
// loads and stores)
typedef uint32_t generate_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 gn_gload(const void *p, uint64_t idx)
{
	const generate_u32x4 x = ((const __attribute__((address_space(1))) generate_u32x4 *)(uintptr_t)p)[idx];
	return uint4{x.x, x.y, x.z, x.w};
}
__device__ __forceinline__ void gn_gstore(uint4 *p, uint64_t idx, uint4 v)
{
	((__attribute__((address_space(1))) generate_u32x4 *)(uintptr_t)p)[idx] = generate_u32x4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ uint64_t gn_lo(uint4 v) { return (uint64_t)v.x | ((uint64_t)v.y << 32); }
__device__ __forceinline__ uint64_t gn_hi(uint4 v) { return (uint64_t)v.z | ((uint64_t)v.w << 32); }
__device__ __forceinline__ uint4 gn_pack(uint64_t lo, uint64_t hi) { return uint4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)}; }
__device__ __forceinline__ uint64_t gn_mask(uint32_t bits) { return bits >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << bits) - 1; }
// the low `bits` (a power of two) bits of the pattern repeated through a 64-bit word
__device__ __forceinline__ uint64_t gn_repeat(uint64_t pattern, uint32_t bits)
{
	pattern &= gn_mask(bits);
	for (uint32_t b = bits; b < 64; b <<= 1) pattern |= pattern << b;
	return pattern;
}
// The runs of 2^log_run bits that start at bit `at` of every 2^log_stride (<= 64) bits of x, pushed together into the low bits: pairs of
// runs are joined, then pairs of pairs (the masks are the same in every lane)
__device__ __forceinline__ uint64_t gn_compress(uint64_t x, uint32_t log_run, uint32_t log_stride, uint32_t at)
{
	uint32_t run = 1u << log_run, stride = 1u << log_stride;
	x = (x >> at) & gn_repeat(gn_mask(run), stride);
	while (stride < 64) {
		x = (x | (x >> (stride - run))) & gn_repeat(gn_mask(2 * run), 2 * stride);
		run *= 2;
		stride *= 2;
	}
	return x;
}
// bits [base, base + 64) of the column whose bits below `index` are set
__device__ __forceinline__ uint64_t gn_ones_below(uint64_t index, uint64_t base)
{
	if (index <= base) return 0;
	return index - base >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << (index - base)) - 1;
}

// a b for b in the low 2^K bits of bw, everything in one 64-bit word (the walk of gf128.hpp's mul_walk on the low word alone)
template <int K>
__device__ __forceinline__ uint64_t gn_walk64(uint64_t a, uint64_t bw)
{
	if constexpr (K == 0)
		return a & (0 - (bw & 1));
	else
		return gn_walk64<K - 1>(a, bw) ^ gn_walk64<K - 1>(mulx64<K - 1>(a), bw >> (1 << (K - 1)));
}
// The product in the field of tower level `level` (3 .. 7) of two of its values (the low 2^level bits of their B128 embedding; the
// product stays there): b byte by byte, a 2^(8 i) times the byte by the walk -- a loop, so that the registers of one byte's walk
// are all that is live.
__device__ __forceinline__ f128 gn_mul(f128 a, f128 b, uint32_t level)
{
	if (level == 7) {
		f128 r = f128_zero();
#pragma unroll 1
		for (uint32_t i = 0; i < 16; i++) r ^= mul_walk<3>(mul_basis(a, 8 * i), ((i & 8) ? b.hi : b.lo) >> (8 * (i & 7)));
		return r;
	}
	uint64_t r = 0;
#pragma unroll 1
	for (uint32_t i = 0; i < (1u << (level - 3)); i++) {
		uint64_t z = a.lo;
		if (i & 1) z = mulx64<3>(z);
		if (i & 2) z = mulx64<4>(z);
		if (i & 4) z = mulx64<5>(z);
		r ^= gn_walk64<3>(z, b.lo >> (8 * i));
	}
	return f128{r, 0};
}

// The thread's elements j0, j0 + 256, ... of a chunk of a column of powers at level K (3 .. 7, the same in every lane): tab[b] = base^(2^b).
__device__ __forceinline__ void gn_powers_chunk(const f128 *__restrict__ tab, uint32_t K, uint32_t n_bits, uint64_t j0, uint64_t len, uint4 *out)
{
	const uint32_t V = 1u << (7 - K); // values of an element
	if (j0 >= len) return;
	const uint64_t i0 = j0 << (7 - K);
	f128 first = f128_one();
#pragma unroll 1
	for (uint32_t b = 7 - K; b < n_bits; b++) {
		const f128 y = gn_mul(first, tab[b], K);
		if ((i0 >> b) & 1) first = y;
	}
	const f128 g = tab[0], stride = tab[8 + 7 - K]; // one value on; 256 elements on
	f128 cur = first;
	uint64_t lo = cur.lo, hi = cur.hi;
#pragma unroll 1
	for (uint32_t idx = 1; idx <= kGnPerThread * V; idx++) {
		const uint32_t t = idx & (V - 1), q = idx >> (7 - K);
		if (t == 0) { // element q - 1 is complete
			const uint64_t j = j0 + 256 * (uint64_t)(q - 1);
			if (j < len) gn_gstore(out, j, gn_pack(lo, hi));
			if (q == kGnPerThread) break;
		}
		cur = gn_mul(t == 0 ? first : cur, t == 0 ? stride : g, K);
		if (t == 0) {
			first = cur;
			lo = cur.lo;
			hi = cur.hi;
		} else if ((t << K) < 64) {
			lo |= cur.lo << (t << K);
		} else {
			hi |= cur.lo << ((t << K) - 64);
		}
	}
}

__global__ __launch_bounds__(256) void k_generate_columns(const generate_job *__restrict__ jobs, uint32_t n_jobs, const f128 *__restrict__ powers)
{
	const uint32_t tid = threadIdx.x, u = blockIdx.x;
	const generate_job &jb = jobs[find_job(jobs, n_jobs, u)];
	const void *in = (const void *)uni64((uint64_t)jb.in);
	uint4 *out = (uint4 *)uni64((uint64_t)jb.out);
	const uint64_t len = uni64(jb.out_elems), m0 = uni64(jb.m0), m1 = uni64(jb.m1);
	const uint32_t p0 = uni32(jb.p0), p1 = uni32(jb.p1), p2 = uni32(jb.p2), p3 = uni32(jb.p3), form = uni32(jb.form);
	const uint32_t unit_elems = uni32(jb.unit_elems);
	const uint64_t unit_first = (uint64_t)(u - uni32(jb.start)) * unit_elems;
#define GN_AT(q) (j[q] < len ? j[q] : len - 1)
#pragma unroll 1
	for (uint32_t c = 0; c < unit_elems / kGnChunkElems; c++) { // the unit, a chunk of 256 * kGnPerThread elements at a time: the job lookup above is paid once
		const uint64_t base = unit_first + c * kGnChunkElems + tid;
		if (base - tid >= len) break;
		uint64_t j[kGnPerThread]; // the element each store goes to; loads use the clamped index
		uint4 r[kGnPerThread];
#pragma unroll
		for (uint32_t q = 0; q < kGnPerThread; q++) j[q] = base + 256 * q;

		switch (form) {
		case kGnProjElem: {
			const uint64_t in_run = ((uint64_t)1 << p0) - 1;
#pragma unroll
			for (uint32_t q = 0; q < kGnPerThread; q++) {
				const uint64_t at = GN_AT(q);
				r[q] = gn_gload(in, m0 + (at & in_run) + ((at >> p0) << p1));
			}
			break;
		}
		case kGnProjField:
		case kGnProjSpread: {
			// an output element is 2^log_pieces pieces of 128 >> log_pieces (<= 64) bits, piece k made from ONE input element
			const bool field = form == kGnProjField;
			const uint32_t log_pieces = field ? 7 - p0 : p2, piece_bits = 128u >> log_pieces, step = field ? p1 : 0, half = field ? 0 : 64u >> p2;
			const uint64_t run = gn_mask(1u << p0);
			uint64_t lo[kGnPerThread], hi[kGnPerThread], e[kGnPerThread];
#pragma unroll
			for (uint32_t q = 0; q < kGnPerThread; q++) {
				lo[q] = hi[q] = 0;
				e[q] = GN_AT(q) << log_pieces;
			}
#pragma unroll 1
			for (uint32_t k = 0; k < (1u << log_pieces); k += 2) {
				uint4 a[kGnPerThread], b[kGnPerThread];
#pragma unroll
				for (uint32_t q = 0; q < kGnPerThread; q++) {
					a[q] = gn_gload(in, m0 + ((e[q] + k) << step));
					b[q] = gn_gload(in, m0 + ((e[q] + k + 1) << step));
				}
				const uint32_t bit = k * piece_bits; // pieces k and k + 1 lie in one 64-bit word, or are one word each
#pragma unroll
				for (uint32_t q = 0; q < kGnPerThread; q++) {
					uint64_t va, vb;
					if (field) {
						va = (((p2 & 64) ? gn_hi(a[q]) : gn_lo(a[q])) >> (p2 & 63)) & run;
						vb = (((p2 & 64) ? gn_hi(b[q]) : gn_lo(b[q])) >> (p2 & 63)) & run;
					} else {
						va = gn_compress(gn_lo(a[q]), p0, p1, p3) | (gn_compress(gn_hi(a[q]), p0, p1, p3) << half);
						vb = gn_compress(gn_lo(b[q]), p0, p1, p3) | (gn_compress(gn_hi(b[q]), p0, p1, p3) << half);
					}
					if (piece_bits == 64) {
						lo[q] = va;
						hi[q] = vb;
					} else if (bit & 64) {
						hi[q] |= (va | (vb << piece_bits)) << (bit & 63);
					} else {
						lo[q] |= (va | (vb << piece_bits)) << bit;
					}
				}
			}
#pragma unroll
			for (uint32_t q = 0; q < kGnPerThread; q++) r[q] = gn_pack(lo[q], hi[q]);
			break;
		}
		case kGnConst: {
#pragma unroll
			for (uint32_t q = 0; q < kGnPerThread; q++) r[q] = gn_pack(m0, m1);
			break;
		}
		case kGnStep: {
#pragma unroll
			for (uint32_t q = 0; q < kGnPerThread; q++) r[q] = gn_pack(gn_ones_below(m0, 128 * j[q]) ^ m1, gn_ones_below(m0, 128 * j[q] + 64) ^ m1);
			break;
		}
		case kGnSelect: {
			const uint64_t word = m0 >> 6, bit = (uint64_t)1 << (m0 & 63);
#pragma unroll
			for (uint32_t q = 0; q < kGnPerThread; q++) r[q] = gn_pack(2 * j[q] == word ? bit : 0, 2 * j[q] + 1 == word ? bit : 0);
			break;
		}
		case kGnIncrement: {
#pragma unroll
			for (uint32_t q = 0; q < kGnPerThread; q++) {
				if (p0 == 128)
					r[q] = gn_pack(j[q], 0);
				else // (p1 = log2 of the values of a word: word W starts at value W << p1)
					r[q] = gn_pack(gn_repeat((2 * j[q]) << p1, p0) | m0, gn_repeat((2 * j[q] + 1) << p1, p0) | m0);
			}
			break;
		}
		default: { // kGnPowers: stores its elements itself
			const f128 *tab = powers + uni32(jb.table);
			gn_powers_chunk(tab, p0, p1, base, len, out);
			continue;
		}
		}
#pragma unroll
		for (uint32_t q = 0; q < kGnPerThread; q++)
			if (j[q] < len) gn_gstore(out, j[q], r[q]);
	}
#undef GN_AT
}

hipError_t launch_generate_columns(hipStream_t s, const generate_job *d_jobs, uint32_t n_jobs, const f128 *d_powers, uint32_t total_units)
{
	if (n_jobs == 0 || total_units == 0) return hipSuccess;
	hipLaunchKernelGGL(k_generate_columns, dim3(total_units), dim3(256), 0, s, d_jobs, n_jobs, d_powers);
	return hipGetLastError();
}

} // namespace bn
