// binius_amd/csrc/kernels_group.hip -- ONE launch for a whole batch round of bivariate sumchecks: every product claim of every
// prover that is ready becomes a JOB of the launch -- the fold of the claim's two multilinears fused with the evaluation of the
// next round polynomial (kind 0), or the evaluation alone (kind 1) -- and the launch returns the RAW sums of all jobs.
//
//   kind 0   a'[i] = a[i] + z (a[i + N/2] - a[i]), likewise b'          (extrapolate_line, compute/src/layer.rs:421)
//            S_1   = sum_{j < N/4} a'[j + N/4] b'[j + N/4]
//            S_inf = sum_{j < N/4} (a'[j] + a'[j + N/4]) (b'[j] + b'[j + N/4])
//   kind 1   S_1 = sum_j a_1[j] b_1[j], S_inf = sum_j (a_0[j] + a_1[j]) (b_0[j] + b_1[j]) over the halves a_0 | a_1, b_0 | b_1 as they are
//   kind 2   two plain inner products of rows: S[slot] = sum_j A[j] B[j], S[slot + 1] = sum_j C[j] D[j]  (the final sums of compiled
//            circuits for all evaluation points of an old-HAL request in one launch, abi_hal.cpp; C = null: one product;
//            B or D = null: the all-ones row, i.e. the plain sum of A or C)
//   kind 3   the fold of kind 0 for one or two arrays and nothing else (an array that several claims share is folded ONCE, by a
//            kind-0 job of one of its claims or by a kind-3 job; the other claims over it are kind-1 / kind-4 jobs)
//   kind 4   kind 0 for the FIRST array only: a is folded on the way, b is read as it is (its halves b_0 | b_1, like kind 1) -- a claim
//            whose second multilinear is shared with other claims (piop::prove pairs every committed multilinear of a size with
//            the few ring-switch transparents of that size: a star around each transparent) folds its own array and reads the
//            shared one, already folded by an earlier job of the chain or up to date
//
// Chains.  A kind-1 job may read what a kind-0 / kind-3 job of the SAME launch writes -- the folds are in place, so a workgroup
// that evaluated such a claim while another one folded the array would read half-folded memory.  Jobs that depend on each other
// therefore form a chain: ONE set of workgroups runs them one after the other, each workgroup on the same tiles in every job,
// the folding jobs first.  A workgroup then only ever reads back what it wrote itself: it waits for its stores (vmcnt), meets
// its own waves at a barrier and invalidates its vector cache (the `acquire` flag of the first reading job) -- no grid-wide
// synchronisation, no second launch, and the shared arrays' folds cost no pass of their own.
//
// Why.  The reference's PCS prover issues k product claims over m multilinears per prover and runs several provers front-loaded
// on one ComputeLayer: per batch round  execute(P_1) .. execute(P_p), one challenge, fold(P_1) .. fold(P_p)
// (core/src/piop/prove.rs:271-287, core/src/protocols/sumcheck/prove/front_loaded.rs:122-155,
// v3/bivariate_product.rs:303-408).  kernels_foldeval_fp4.hip fuses exactly ONE claim over two arrays.  Here the workgroups of
// one launch are dealt out to the jobs (job j owns workgroups [wg_begin, wg_begin + wg_count): its own tile order, its own
// nibble table for its own challenge, its own pair of accumulator slots); inside its range a workgroup is the twelve-wave
// workgroup of kernels_foldeval_fp4.hip -- waves 4 .. 11 fold / load and stage a pair of tiles, waves 0 .. 3 run the FP4 Gram
// k-steps of the previous pair (gram_fp4.hpp).  The last workgroup of the LAUNCH (device-scope ticket) copies all accumulator
// slots to the pinned mailbox and re-zeroes them; the batch coefficients (value = init + sum_c alpha^c S_c,
// cpu/layer.rs:512) are applied by the host, which keeps the kernel independent of the caller's recipe -- so the sums of a
// prover whose execute() has not been called yet can be computed in the same launch (abi_group.cpp).
//
// Algorithmic bytes per job: kind 0 read 16 * 2 * N + write 8 * 2 * N = 48 N (24 * m * N summed over a prover's disjoint claims);
// kind 1 read 16 * 2 * (N / 2) = 16 N; kind 3 24 N per array; kind 4 24 N + 8 N.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <cstring>
#include <queue>
#include <vector>

#include "ctable.hpp"
#include "gram_fp4.hpp"

namespace bn {

using namespace gram4;

namespace {

typedef unsigned int gq_v4u __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 gq_load(const uint4 *p)
{
	if constexpr (NT) {
		const gq_v4u v = __builtin_nontemporal_load(reinterpret_cast<const gq_v4u *>(p));
		return uint4{v.x, v.y, v.z, v.w};
	} else {
		return *p;
	}
}
template <bool NT>
__device__ __forceinline__ void gq_store(uint4 *p, uint4 r)
{
	if constexpr (NT) {
		const gq_v4u v = {r.x, r.y, r.z, r.w};
		__builtin_nontemporal_store(v, reinterpret_cast<gq_v4u *>(p));
	} else {
		*p = r;
	}
}

constexpr unsigned kGramWaves = 4;  // waves 0 .. 3: the Gram k-steps (one per SIMD)
constexpr unsigned kFoldGroups = 2; // waves 4 .. 11: two groups of four waves, a tile per group
constexpr unsigned kThreads = 64 * kGramWaves * (1 + kFoldGroups);

// The kernel arguments.  The job table itself is NOT among them (256 jobs of 96 bytes: six times what a kernel-argument block
// holds): it lies in pinned, device-mapped memory (internal.hpp group_tables) that the host fills right before the launch, and
// a workgroup reads the one job it works on -- and the followers of its chain -- from there with scalar loads.  Which job that
// is comes from head_of_wg: two 16-bit job numbers per word, indexed by workgroup.
struct group_kargs {
	uint32_t head_of_wg[kGroupMaxGrid / 2];
	const group_job *table;
	f128 *S;           // accumulator slots (zero before the launch, zero after it)
	f128 *vals;        // pinned: [0, n_slots) the raw sums
	f128 *mail;        // pinned mailbox: word 64 the sequence number
	unsigned *counter; // device-scope ticket (zero between launches)
	uint64_t seq;
	uint32_t n_jobs, n_slots, prio, pad;
};

// read-only views for SCALAR loads with a run-time index: the kernel-argument segment and the pinned job table are both memory
// nobody writes while the launch runs (address space 4 = constant: a load through it with a uniform address is an s_load, its
// result lives in scalar registers -- through a generic pointer the compiler would issue vector loads and carry every pointer
// of the job as a 64-bit vector value through the tile loops)
typedef const group_job __attribute__((address_space(4))) *cjob_ptr;
typedef const uint32_t __attribute__((address_space(4))) *cu32_ptr;
__device__ __forceinline__ cu32_ptr kernarg_words()
{
#if defined(__HIP_DEVICE_COMPILE__)
	return (cu32_ptr)__builtin_amdgcn_kernarg_segment_ptr();
#else
	return nullptr;
#endif
}
__device__ __forceinline__ cjob_ptr as_const_jobs(const group_job *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return (cjob_ptr)p;
#else
	(void)p;
	return nullptr;
#endif
}

} // namespace

// what a workgroup needs to know about its job and its share of the job's tiles (uniform)
struct group_wg {
	const char *X0[2], *X1[2];
	char *OUT[2];
	f128 z;
	uint64_t n;
	uint32_t tbase, tstride, tlimit, t0;
	uint32_t adj; // 1: the two fold groups take ADJACENT tiles (2 p, 2 p + 1) of the workgroup's p-th pair instead of tiles a stride apart
};

// The loops of one workgroup for a job of kind KIND (0: fold + evaluate, 1: evaluate).  A function template per kind -- and not
// a run-time `kind` inside one loop -- because the loaded elements must live in registers: with both kinds' uses of x0 / x1 in
// one body the compiler keeps the two arrays in scratch memory and every tile pays 128 bytes of scratch stores and loads per
// lane (measured: the launch at half the rate of kernels_foldeval_fp4.hip).  Leaves the parity words of the Gram waves in Gc.
template <int KIND, bool FULL, bool NT>
__device__ __forceinline__ void group_loops(const group_wg &w, uint32_t *T_dyn, ctable_smem &tab, gram_parity &Gc, uint32_t prio, bool build)
{
	constexpr bool kFolds = KIND == 0 || KIND == 3 || KIND == 4; // the job folds its arrays (KIND 3: and nothing else -- no staging, no Gram work, no sums;
	                                                                // KIND 4: its first array only, the second is read as it is)
	constexpr bool kTwoAhead = KIND == 1 || KIND == 2;
	// (the thread index behind an opaque move: everything derived from it -- roles, lane offsets -- is recomputed per job of a chain
	// instead of being hoisted out of the kernel's job loop and kept in registers across all four loop bodies)
	unsigned tx = threadIdx.x;
	asm volatile("" : "+v"(tx));
	const unsigned lane = tx & 63;
	const unsigned wave = __builtin_amdgcn_readfirstlane(tx >> 6);
	const bool folds = wave >= kGramWaves;
	const unsigned grp = folds ? (wave - kGramWaves) >> 2 : 0;   // fold group: which tile of the pair
	const unsigned ftid = (tx - 64 * kGramWaves) & 255; // the lane's point inside its tile (fold waves)
	const uint64_t n = w.n;
	const uint32_t tbase = w.tbase, tstride = w.tstride, tlimit = w.tlimit, t0 = w.t0;
	// iteration variable `it` = t0, t0 + step, ... < limit; tile of fold group g in iteration it
	const uint32_t adj = w.adj, step = adj ? tstride : 2 * tstride, limit = adj ? (tlimit + 1) >> 1 : tlimit;
	auto tile_of = [&](uint32_t it, uint32_t g) { return adj ? 2 * it + g : it + g * tstride; };

	// quadrant q = 2 * side + half.  KIND 0: x0[q] / x1[q] = the two elements the fold of (side, half) reads; KIND 1: x0[q] = the
	// element of (side, half) itself.
	uint4 x0[4], x1[kFolds ? 4 : 1];
	const uint32_t voff = ftid * 16u;
	auto lane_off = [&]() { // (kernels_foldeval_fp4.hip: keeps the lane offset out of a loop-invariant 64-bit vector base)
		uint32_t v = voff;
		asm volatile("" : "+v"(v));
		return v;
	};
	uint32_t vo = lane_off();
	auto in_range = [&](uint32_t t) { return FULL || (uint64_t)(tbase + t) * kTP + ftid < n; };
	// KIND 1 keeps TWO tiles of loads in flight per fold group (x0: the tile after this one, xb: the one after that): with nothing to
	// compute between a tile's loads and its staging, one tile in flight is 32 KiB per CU and the launch sits at the memory
	// latency (2.1 TB/s measured at 2^25 points per claim); KIND 0 has 64 KiB of loads per CU in flight with one tile per group
	uint4 xb[kTwoAhead ? 4 : 1];
	auto load_into = [&](uint4 *dst0, uint32_t t, int q) {
		const uint32_t o = in_range(t) ? vo : 0u; // (a lane past the end reads the tile's first element: in range, never used)
		if constexpr (kFolds) {
			if (KIND == 3 && q >= 2 && w.X0[1] == nullptr) return; // (uniform) a fold-only job of ONE array
			if (KIND == 4 && q >= 2) { // the second array as it is: X0 = its lower half (evaluations at 0), X1 = its upper half
				const uint64_t e1 = (uint64_t)(tbase + t) * kTP * 16;
				dst0[q] = gq_load<NT>(reinterpret_cast<const uint4 *>((q & 1 ? w.X1[1] : w.X0[1]) + e1 + o));
				return;
			}
			const uint64_t e = ((q & 1 ? n : 0) + (uint64_t)(tbase + t) * kTP) * 16; // (uniform)
			dst0[q] = gq_load<NT>(reinterpret_cast<const uint4 *>(w.X0[q >> 1] + e + o));
			x1[q] = gq_load<NT>(reinterpret_cast<const uint4 *>(w.X1[q >> 1] + e + o));
		} else if constexpr (KIND == 1) {
			const uint64_t e1 = (uint64_t)(tbase + t) * kTP * 16;
			dst0[q] = gq_load<NT>(reinterpret_cast<const uint4 *>((q & 1 ? w.X1[q >> 1] : w.X0[q >> 1]) + e1 + o));
		} else {
			// rows A, B, C, D = x0[0], x0[1], x1[0], x1[1]; an absent second product reads the first one's rows (its sum is never looked at)
			const uint64_t e1 = (uint64_t)(tbase + t) * kTP * 16;
			const bool second = q >= 2 && w.X1[0] != nullptr; // (uniform)
			const char *row = q < 2 ? w.X0[q] : (second ? w.X1[q - 2] : w.X0[q - 2]);
			if (row) // (uniform) a null second factor is the all-ones row: the sum of the first factor, with nothing loaded for it
				dst0[q] = gq_load<NT>(reinterpret_cast<const uint4 *>(row + e1 + o));
			else
				dst0[q] = uint4{1, 0, 0, 0};
		}
	};
	auto load1 = [&](uint32_t t, int q) { load_into(x0, t, q); };
	const uint32_t tm0 = tile_of(t0, grp); // this fold group's first tile
	if (folds && t0 < limit && tm0 < tlimit) {
#pragma unroll
		for (int q = 0; q < 4; q++)
			load1(tm0, q);
		if constexpr (kTwoAhead) {
			const uint32_t tm1 = (t0 + step < limit && tile_of(t0 + step, grp) < tlimit) ? tile_of(t0 + step, grp) : tm0;
#pragma unroll
			for (int q = 0; q < 4; q++)
				load_into(xb, tm1, q);
		}
	}
	if constexpr (kFolds) {
		if (build) ctable_build(tab, w.z); // (uniform; the loads above are in flight meanwhile; ends with a barrier)
	}
	if (folds) {
		switch (prio & 3) { // the fold waves issue ahead of the Gram wave of their SIMD (kernels_foldeval_fp4.hip)
		case 1: __builtin_amdgcn_s_setprio(1); break;
		case 2: __builtin_amdgcn_s_setprio(2); break;
		case 3: __builtin_amdgcn_s_setprio(3); break;
		default: break;
		}
		const stage4_role sr = make_stage4_role(ftid);
		uint32_t *Tn = T_dyn + grp * kTile4W;
		unsigned buf = 0;
		// one pair of tiles: `cur` holds this group's tile, loaded one (KIND 0) or two (KIND 1) iterations ago, and is refilled for
		// the iteration that will use it next
		auto pair_step = [&](uint32_t t, uint4 *cur) {
			const uint32_t tm = tile_of(t, grp);
			if (tm < tlimit) { // (uniform; false only for group 1 on an odd last pair)
				// the last iteration(s) re-request their own tile (cache hits) instead of branching around the loads
				constexpr uint32_t kAhead = kTwoAhead ? 2 : 1; // iterations ahead
				const uint32_t ta = t + kAhead * step;
				const uint32_t tn = (ta < limit && tile_of(ta, grp) < tlimit) ? tile_of(ta, grp) : tm;
				vo = lane_off();
				const bool ok = in_range(tm);
				uint4 f[4];
				if constexpr (kFolds) {
					const uint64_t pt16 = (uint64_t)(tbase + tm) * kTP * 16; // (uniform)
					const int nq = (KIND == 3 && w.X0[1] == nullptr) ? 2 : 4; // (uniform)
#pragma unroll
					for (int q = 0; q < 4; q++) {
						if (q >= nq) break;
						if (KIND == 4 && q >= 2)
							f[q] = x0[q];
						else
							f[q] = ctable_mul_acc<8, true>(tab, xor4(x0[q], x1[q]), x0[q]);
						load1(tn, q); // this quadrant of the group's next tile flies from here on
					}
					if (FULL || ok) {
#pragma unroll
						for (int q = 0; q < 4; q++) {
							if (q >= nq || (KIND == 4 && q >= 2)) break;
							gq_store<NT>(reinterpret_cast<uint4 *>(w.OUT[q >> 1] + (q & 1 ? n * 16 : 0) + pt16 + vo), f[q]);
						}
					}
				} else {
#pragma unroll
					for (int q = 0; q < 4; q++) {
						f[q] = cur[q];
						load_into(cur, tn, q);
					}
				}
				if constexpr (KIND != 3) {
					if (!FULL && !ok) {
#pragma unroll
						for (int q = 0; q < 4; q++)
							f[q] = uint4{0, 0, 0, 0}; // points past the end carry zeros
					}
				}
				if constexpr (KIND == 3) {
					// (nothing is staged)
				} else if constexpr (KIND == 2) {
					// sets 0 / 1 = the first product's rows, sets 2 / 3 = the second's
					stage4_elem(Tn, sr, 0, f[0]);
					stage4_elem(Tn, sr, 1, f[1]);
					stage4_elem(Tn, sr, 2, f[2]);
					stage4_elem(Tn, sr, 3, f[3]);
				} else {
					// half 1 is the evaluation at 1, half 0 its partner: sets 0 / 1 = u, v at 1; sets 2 / 3 = u, v at infinity
					stage4_elem(Tn, sr, 0, f[1]);
					stage4_elem(Tn, sr, 2, xor4(f[1], f[0]));
					stage4_elem(Tn, sr, 1, f[3]);
					stage4_elem(Tn, sr, 3, xor4(f[3], f[2]));
				}
			}
			if constexpr (KIND != 3) __syncthreads(); // the pair is staged; the Gram waves are done with the buffer this wave writes next
			buf ^= 1;
			Tn = T_dyn + (buf * kFoldGroups + grp) * kTile4W;
		};
		if constexpr (kFolds) {
			for (uint32_t t = t0; t < limit; t += step) pair_step(t, x0);
		} else { // (KIND 1, 2: two tiles in flight)
			for (uint32_t t = t0; t < limit;) {
				pair_step(t, x0);
				t += step;
				if (t >= limit) break;
				pair_step(t, xb);
				t += step;
			}
		}
		__builtin_amdgcn_s_setprio(0);
	} else if constexpr (KIND != 3) {
		const gram4_role gr = make_gram4_role(wave, lane);
		v16f acc[kAccTiles];
		acc4_zero(acc);
		unsigned buf = 0;
		for (uint32_t t = t0; t < limit; t += step) {
			__syncthreads();
			const uint32_t *Tp = T_dyn + buf * kFoldGroups * kTile4W;
			gram4_tile(Tp, gr, acc);
			if (tile_of(t, 1) < tlimit) gram4_tile(Tp + kTile4W, gr, acc);
			buf ^= 1;
		}
		parity4(acc, gr, wave, lane, Gc);
	}
}

template <bool FULL, bool NT>
__global__ __launch_bounds__(kThreads, 1) void k_group_fp4(group_kargs ga)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t T_dyn[]; // 2 buffers x 2 tiles of FP4 operands
	__shared__ ctable_smem tab;
	__shared__ gram_parity Gc;
	const unsigned lane = threadIdx.x & 63;
	const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

	// ---- this workgroup's job (uniform): the head of its chain, or the lone job, from the table in the kernel arguments; the job
	// itself (and the followers of the chain) from the pinned table
	static_assert(offsetof(group_kargs, head_of_wg) == 0, "the head-of-workgroup table leads the kernel-argument block");
	const uint32_t hw = kernarg_words()[blockIdx.x >> 1];
	const unsigned ji = (blockIdx.x & 1) ? hw >> 16 : hw & 0xFFFFu;
	const cjob_ptr head = as_const_jobs(ga.table) + ji;
	const uint32_t G = head->wg_count, b = blockIdx.x - head->wg_begin;
	const bool xcd_order = (G & 7) == 0 && (head->wg_begin & 7) == 0;
	const unsigned n_sub = 1 + head->chain;
	__shared__ uint64_t z3[2][3];
	__shared__ f128 s_loc[2];
	__shared__ unsigned is_last;
	const unsigned tid = threadIdx.x;
	f128 z_built{0, 0};
	bool have_table = false;
	for (unsigned sub = 0; sub < n_sub; sub++) {
		const cjob_ptr jb = head + sub;
		if (jb->acquire) {
			// this workgroup's own stores of the chain's earlier jobs (folded arrays, in place) are read back by this job: all of
			// them have reached the L2 (vmcnt), and the vector cache forgets the lines it loaded before they were written
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__syncthreads();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
		}
		group_wg w;
		w.n = jb->n; // evaluation points of the job
		w.z = f128{jb->z.lo, jb->z.hi};
		for (int sd = 0; sd < 2; sd++) {
			w.X0[sd] = reinterpret_cast<const char *>(jb->x0[sd]);
			w.X1[sd] = reinterpret_cast<const char *>(jb->x1[sd]);
			w.OUT[sd] = reinterpret_cast<char *>(jb->out[sd]);
		}
		const uint32_t n_tiles = (uint32_t)(FULL ? w.n / kTP : (w.n + kTP - 1) / kTP);
		// tile order inside the job's range: as kernels_foldeval_mfma.hip (XCD x = blockIdx.x & 7 takes the x-th contiguous eighth of
		// the job's tiles) when the range starts on a multiple of eight workgroups and is a multiple of eight long
		w.tbase = 0;
		w.tstride = G;
		w.tlimit = n_tiles;
		w.t0 = b;
		if (xcd_order) {
			const uint32_t chunk = (n_tiles + 7) >> 3;
			w.tbase = (b & 7) * chunk;
			w.tstride = G >> 3;
			w.t0 = b >> 3;
			w.tlimit = w.tbase >= n_tiles ? 0 : (n_tiles - w.tbase < chunk ? n_tiles - w.tbase : chunk);
		}
		w.adj = (ga.prio >> 2) & 1;
		const uint32_t kind = jb->kind; // (uniform)
		const bool build = !have_table || !(z_built == w.z);
		if (kind == 0 || kind == 3 || kind == 4) {
			z_built = w.z;
			have_table = true;
		}
		if (kind == 0)
			group_loops<0, FULL, NT>(w, T_dyn, tab, Gc, ga.prio, build);
		else if (kind == 4)
			group_loops<4, FULL, NT>(w, T_dyn, tab, Gc, ga.prio, build);
		else if (kind == 1)
			group_loops<1, FULL, NT>(w, T_dyn, tab, Gc, ga.prio, false);
		else if (kind == 2)
			group_loops<2, FULL, NT>(w, T_dyn, tab, Gc, ga.prio, false);
		else
			group_loops<3, FULL, NT>(w, T_dyn, tab, Gc, ga.prio, build);
		if (kind == 3) { // (no sums; the waves that had nothing to do must not rebuild the table under the folding ones)
			__syncthreads();
			continue;
		}

		// ---- parity words -> the job's two sums -> its accumulator slots
		__syncthreads();
		// column n' = 32 h + n of matrix (pr, s) as a GF(2^64) element (bit p = G[p][n']); z = sum_n' col * e_n'  (gram.hpp tail_finish)
		for (unsigned task = wave; task < 6; task += kThreads / 64) {
			const unsigned pr = task / 3, s = task - 3 * pr;
			const unsigned h = lane >> 5, nn = lane & 31;
			auto spread = [](uint32_t x) { return (x & 0xFu) | ((x & 0xF0u) << 4) | ((x & 0xF00u) << 8) | ((x & 0xF000u) << 12); };
			const uint32_t *g0 = Gc[2 * pr + h][2 * s], *g1 = Gc[2 * pr + h][2 * s + 1];
			const uint32_t lo = spread(g0[nn]) | (spread(g0[nn + 32]) << 4);
			const uint32_t hi = spread(g1[nn]) | (spread(g1[nn + 32]) << 4);
			uint64_t z = mul_basis64((uint64_t)lo | ((uint64_t)hi << 32), lane);
#pragma unroll
			for (int mm = 32; mm >= 1; mm >>= 1)
				z ^= __shfl_xor(z, mm, 64);
			if (lane == 0) z3[pr][s] = z;
		}
		__syncthreads();
		if (tid < 2) s_loc[tid] = kara64(z3[tid][0], z3[tid][1], z3[tid][2]);
		__syncthreads();
		if (tid < 4) {
			const uint64_t v = reinterpret_cast<const uint64_t *>(s_loc)[tid];
			if (v) atomicXor(reinterpret_cast<unsigned long long *>(ga.S + jb->slot) + tid, (unsigned long long)v);
		}
	}
	// ---- the last workgroup of the launch publishes ALL slots
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	if (tid == 0) {
		const unsigned tk = atomicAdd(ga.counter, 1u);
		is_last = (tk == gridDim.x - 1) ? 1u : 0u;
	}
	__syncthreads();
	if (is_last) {
		// (everything below happens in wave 0, whose drain orders the value stores before the sequence word -- posted writes to one
		// destination keep their order; finalize.hpp)
		if (tid < 64) {
			for (unsigned i = tid; i < ga.n_slots; i += 64) {
				f128 v;
				v.lo = __hip_atomic_load(&ga.S[i].lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				v.hi = __hip_atomic_load(&ga.S[i].hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__hip_atomic_store(&ga.vals[i].lo, v.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
				__hip_atomic_store(&ga.vals[i].hi, v.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
				__hip_atomic_store(&ga.S[i].lo, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__hip_atomic_store(&ga.S[i].hi, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		}
		if (tid == 0) {
			__hip_atomic_store(&ga.mail[64].lo, ga.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
			__hip_atomic_store(ga.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}

// The launch: the planner (group_plan.hpp) deals the workgroups out to the jobs and orders the table; the table goes to the pinned
// block, the kernel arguments are filled and one of three instantiations is launched.
namespace {
// read once per process
struct group_knobs {
	uint32_t prio, adj_tiles;
	int nt_log2;      // streaming accesses from 4 << nt_log2 elements touched
	bool pack_forced; // BN_GROUP_PACK_U (measurement builds: that many super-units; -1: one unit per job -- tools/r06_pack_sweep.sh)
	int pack_u;
	bool prof;        // BN_GROUP_PROF (diagnostic: host time of launch_group by step, and of the runtime's launch call itself)
	group_knobs()
	{
		auto knob = [](const char *name, int unset) {
			const char *e = bn::settled_knob(name);
			return e ? atoi(e) : unset;
		};
		prio = (uint32_t)knob("BN_FE_FP4_PRIO", 3) & 3u;
		adj_tiles = (uint32_t)(knob("BN_GROUP_ADJ", 0) != 0); // (round-5 A/B, profiles/DEAD_ENDS.md: adjacent tiles per pair of fold groups -- no difference)
		// (the single-claim kernels' threshold is 2^25 elements per array = 2^27 elements touched; BN_GROUP_NT_MIN_LOG2, measurement
		// builds: the same threshold for launches of the group kernel only; A/B of round 6 within the noise in both directions,
		// profiles/r06/README.md)
		const int nt_group_log2 = knob("BN_GROUP_NT_MIN_LOG2", -1);
		nt_log2 = nt_group_log2 >= 0 ? nt_group_log2 : knob("BN_FE_NT_MIN_LOG2", 25);
		const char *pack = bn::settled_knob("BN_GROUP_PACK_U");
		pack_forced = pack != nullptr;
		pack_u = pack ? atoi(pack) : 0;
		prof = getenv("BN_GROUP_PROF") != nullptr;
	}
};
// BN_GROUP_PROF: laps 0 .. 2 in front of the launch call; lap 3 the call itself, from launch_begin() to the end of the scope, which
// completes a counted call; one line on stderr every 64 of them
struct group_prof {
	typedef std::chrono::steady_clock clock;
	const bool on;
	bool launching = false;
	clock::time_point t;
	explicit group_prof(bool on_) : on(on_), t(on_ ? clock::now() : clock::time_point{}) {}
	void lap(int i)
	{
		static double us[4] = {0, 0, 0, 0};
		static uint64_t calls = 0;
		if (!on) return;
		const auto now = clock::now();
		us[i] += std::chrono::duration<double, std::micro>(now - t).count();
		t = now;
		if (i == 3 && (++calls & 63) == 0)
			fprintf(stderr, "[bn group prof] hipLaunchKernel of the group kernel: %.2f us per call over %llu calls; in front of it, us per call: weights + decision %.2f, dealing %.2f, table copy %.2f\n",
			        us[3] / calls, (unsigned long long)calls, us[0] / calls, us[1] / calls, us[2] / calls);
	}
	void launch_begin()
	{
		launching = on;
		if (on) t = clock::now();
	}
	~group_prof()
	{
		if (launching) lap(3);
	}
};
hipError_t plan_error(group_plan::status_t st) { return st == group_plan::ok ? hipSuccess : st == group_plan::invalid ? hipErrorInvalidValue : hipErrorNotSupported; }
static_assert(kGroupTilePoints == (uint32_t)kTP, "the planner counts the kernel's tiles");
} // namespace

hipError_t launch_group(hipStream_t s, int n_cu, const group_job *jobs_in, uint32_t n_jobs, uint32_t n_slots, f128 *d_S, f128 *d_vals, f128 *d_mail,
                        unsigned *d_counter, uint64_t seq, group_job *h_table, const group_job *d_table)
{
	if (!h_table || !d_table) return hipErrorNotSupported;
	static const group_knobs knobs;
	static thread_local group_planner planner;
	group_prof prof(knobs.prof);
	const group_plan &plan = planner.decide(jobs_in, n_jobs, n_slots, n_cu, knobs.pack_forced, knobs.pack_u); // (the planner's: deal() completes it)
	if (plan.status != group_plan::ok) return plan_error(plan.status);
	prof.lap(0);
	if (planner.deal().status != group_plan::ok) return plan_error(plan.status);
	// (the table is put together in ordinary memory and goes to the pinned block in one sequential copy: the block is written once,
	// front to back, never read or patched by the host)
	prof.lap(1);
	std::memcpy(h_table, plan.table, (size_t)n_jobs * sizeof(group_job));
	__atomic_thread_fence(__ATOMIC_SEQ_CST); // (the table is in memory before the doorbell rings)
	prof.lap(2);
	group_kargs ga;
	std::memcpy(ga.head_of_wg, plan.head_of_wg, sizeof(ga.head_of_wg));
	ga.table = d_table;
	ga.S = d_S;
	ga.vals = d_vals;
	ga.mail = d_mail;
	ga.counter = d_counter;
	ga.seq = seq;
	ga.n_jobs = n_jobs;
	ga.n_slots = n_slots;
	ga.prio = knobs.prio | (knobs.adj_tiles << 2);
	ga.pad = 0;
	constexpr unsigned lds = 2 * kFoldGroups * kTile4W * 4;
	for (const void *fn : {reinterpret_cast<const void *>(&k_group_fp4<false, false>), reinterpret_cast<const void *>(&k_group_fp4<true, false>),
	                       reinterpret_cast<const void *>(&k_group_fp4<true, true>)}) {
		const hipError_t e = func_lds_limit(fn, lds);
		if (e != hipSuccess) return e;
	}
	prof.launch_begin();
	if (group_plan_streams(plan, knobs.nt_log2))
		hipLaunchKernelGGL((k_group_fp4<true, true>), dim3(plan.grid), dim3(kThreads), lds, s, ga);
	else if (plan.full)
		hipLaunchKernelGGL((k_group_fp4<true, false>), dim3(plan.grid), dim3(kThreads), lds, s, ga);
	else
		hipLaunchKernelGGL((k_group_fp4<false, false>), dim3(plan.grid), dim3(kThreads), lds, s, ga);
	return hipGetLastError();
}

// ---- host tail of a claim group (abi_group.cpp "hosted sessions") ------------------------------------------------------------
// Hand-over: every array of a prover (count arrays of n elements: at most kGroupTailMaxElems elements in all) goes to the host in the
// power basis of hostmul_clmul.cpp -- after the prover's deferred fold, performed here on the way (fold[j]: y = src0 + z (src0 +
// x1), stored to out[j] as the fold asked) or as it is (x1[j] == null: y = src0[j][i], nothing stored).  Phi is GF(2)-linear:
// one nibble-table product per element (table in device memory, ctable.hpp layout).  The staging is written with plain posted
// stores and validates itself: the last workgroup publishes the XOR over all elements of mirror_mix(value, index) XOR seq in
// mailbox word 66, then the sequence word; the host accepts the staging only when the tag it computes from what it reads is
// that tag (the protocol of kernels_foldeval8.hip's hand-over).
namespace {
__device__ __forceinline__ uint64_t gt_mix(uint64_t lo, uint64_t hi, uint64_t idx)
{
	const unsigned r1 = (unsigned)(idx & 63), r2 = (unsigned)((idx * 7 + 17) & 63);
	return ((lo << r1) | (r1 ? lo >> (64 - r1) : 0)) ^ ((hi << r2) | (r2 ? hi >> (64 - r2) : 0)) ^ (idx + 1) * 0x9E3779B97F4A7C15ull;
}
} // namespace

// (the pointers of the arrays a workgroup touches -- consecutive ones, at most 256 -- come from the pinned pointer table into shared
// memory once per workgroup)
__global__ __launch_bounds__(256) void k_group_mirror(group_mirror_args a)
{
	__shared__ ctable_smem tab;
	__shared__ uint4 phi_T[512];
	__shared__ uint64_t wtag[4];
	__shared__ unsigned is_last;
	__shared__ const void *p_src0[256], *p_x1[256];
	__shared__ void *p_out[256];
	const unsigned tid = threadIdx.x;
	const uint64_t g0 = (uint64_t)blockIdx.x * 256, g = g0 + tid, total = (uint64_t)a.count * a.n;
	const bool act = g < total;
	const uint32_t arr0 = (uint32_t)(g0 / a.n);
	const uint32_t arr = act ? (uint32_t)(g / a.n) : arr0, i = act ? (uint32_t)(g - (uint64_t)arr * a.n) : 0;
	if (arr0 + tid < a.count && (uint64_t)(arr0 + tid) * a.n < g0 + 256) {
		p_src0[tid] = a.ptrs->src0[arr0 + tid];
		p_x1[tid] = a.ptrs->x1[arr0 + tid];
		p_out[tid] = a.ptrs->out[arr0 + tid];
	}
	phi_T[tid] = a.phi_tab[tid];
	phi_T[tid + 256] = a.phi_tab[tid + 256];
	ctable_build(tab, a.z); // (ends with a barrier: phi_T and the pointers are complete too)
	const uint4 *src0 = reinterpret_cast<const uint4 *>(p_src0[arr - arr0]), *x1 = reinterpret_cast<const uint4 *>(p_x1[arr - arr0]);
	uint4 v0{0, 0, 0, 0}, v1{0, 0, 0, 0};
	if (act) {
		v0 = src0[i];
		if (x1) v1 = x1[i];
	}
	uint64_t tag = 0;
	if (act) {
		uint4 y = v0;
		if (x1) {
			y = xor4(v0, ctable_mul(tab, xor4(v0, v1)));
			reinterpret_cast<uint4 *>(p_out[arr - arr0])[i] = y;
		}
		const uint4 py = ctable_mul(*reinterpret_cast<const ctable_smem *>(phi_T), y);
		reinterpret_cast<uint4 *>(a.staging)[g] = py;
		tag = gt_mix((uint64_t)py.x | ((uint64_t)py.y << 32), (uint64_t)py.z | ((uint64_t)py.w << 32), g);
	}
#pragma unroll
	for (int sh = 32; sh >= 1; sh >>= 1) tag ^= __shfl_xor(tag, sh, 64);
	if ((tid & 63) == 0) wtag[tid >> 6] = tag;
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	if (tid == 0) {
		const uint64_t t = wtag[0] ^ wtag[1] ^ wtag[2] ^ wtag[3];
		if (t) atomicXor(reinterpret_cast<unsigned long long *>(a.tag_acc), (unsigned long long)t);
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		const unsigned tk = atomicAdd(a.counter, 1u);
		is_last = tk == gridDim.x - 1 ? 1u : 0u;
		if (is_last) {
			const uint64_t all = __hip_atomic_load(a.tag_acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__hip_atomic_store(a.tag_acc, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__hip_atomic_store(&a.mail[66].lo, all ^ a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__hip_atomic_store(&a.mail[64].lo, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		}
	}
}

hipError_t launch_group_mirror(hipStream_t s, const group_mirror_args &a)
{
	if (a.count == 0 || a.count > (uint32_t)kGroupMaxArrays || a.n == 0 || (uint64_t)a.count * a.n > kGroupTailMaxElems || !a.ptrs || !a.staging || !a.phi_tab ||
	    !a.tag_acc || !a.counter || !a.mail)
		return hipErrorNotSupported;
	__atomic_thread_fence(__ATOMIC_SEQ_CST); // (the pointer table is in memory before the doorbell rings)
	hipLaunchKernelGGL(k_group_mirror, dim3((unsigned)(((uint64_t)a.count * a.n + 255) / 256)), dim3(256), 0, s, a);
	return hipGetLastError();
}

// The device catching up with a hosted prover: out[j][i] = PhiInv(staging[j * n0 + i]), i < n0 -- the first n0 elements of the
// host's folded copies, which are exactly what the folds the caller asked for leave in its buffers (kernels_stream.hip
// k_tail_writeback for any number of arrays).
__global__ __launch_bounds__(256) void k_group_writeback(group_writeback_args a)
{
	__shared__ uint4 T[512];
	__shared__ void *p_out[256];
	const unsigned tid = threadIdx.x;
	const uint64_t g0 = (uint64_t)blockIdx.x * 256, g = g0 + tid, total = (uint64_t)a.count * a.n0;
	const bool act = g < total;
	const uint32_t arr0 = (uint32_t)(g0 / a.n0);
	const uint32_t arr = act ? (uint32_t)(g / a.n0) : arr0, i = act ? (uint32_t)(g - (uint64_t)arr * a.n0) : 0;
	if (arr0 + tid < a.count && (uint64_t)(arr0 + tid) * a.n0 < g0 + 256) p_out[tid] = a.ptrs->out[arr0 + tid];
	uint4 v{0, 0, 0, 0};
	if (act) v = reinterpret_cast<const uint4 *>(a.staging)[g];
	T[tid] = a.phi_inv[tid];
	T[tid + 256] = a.phi_inv[tid + 256];
	__syncthreads();
	if (act) reinterpret_cast<uint4 *>(p_out[arr - arr0])[i] = ctable_mul(*reinterpret_cast<const ctable_smem *>(T), v);
}

hipError_t launch_group_writeback(hipStream_t s, const group_writeback_args &a)
{
	if (a.count == 0 || a.count > (uint32_t)kGroupMaxArrays || a.n0 == 0 || (uint64_t)a.count * a.n0 > kGroupTailMaxElems || !a.ptrs || !a.staging || !a.phi_inv)
		return hipErrorNotSupported;
	__atomic_thread_fence(__ATOMIC_SEQ_CST);
	hipLaunchKernelGGL(k_group_writeback, dim3((unsigned)(((uint64_t)a.count * a.n0 + 255) / 256)), dim3(256), 0, s, a);
	return hipGetLastError();
}

} // namespace bn
