// tools/fp4_probe.hip -- operand / result layout, value decoding and issue rate of v_mfma_scale_f32_32x32x64_f8f6f4 with
// both operands in FP4 (E2M1), probed on the device (no documentation in the image names the lane layout); first of all, whether
// the scale-free form v_mfma_f32_32x32x64_f8f6f4 (both scale arguments 0) gives the same accumulators as scales of 2^0, bit for bit.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/fp4_probe.hip -o tools/fp4_probe
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef int v16i __attribute__((ext_vector_type(16)));

// The two forms of the instruction: SCALED = block scales of 2^0 on both operands (0x7F in every byte of the scale register:
// the 16-byte v_mfma_scale_f32_32x32x64_f8f6f4, whose first word loads the scales), otherwise both scale arguments 0 (the
// 8-byte v_mfma_f32_32x32x64_f8f6f4 cbsz:4 blgp:4 alone).
template <int SCALED>
__device__ __forceinline__ v16f mfma4(v8i x, v8i y, v16f acc)
{
	if (SCALED) return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(x, y, acc, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
	return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(x, y, acc, 4, 4, 0, 0, 0, 0);
}

template <int SCALED>
__global__ void k_one(const uint32_t *a, const uint32_t *b, float *c)
{
	const unsigned l = threadIdx.x;
	v8i x = {(int)a[4 * l], (int)a[4 * l + 1], (int)a[4 * l + 2], (int)a[4 * l + 3], 0, 0, 0, 0};
	v8i y = {(int)b[4 * l], (int)b[4 * l + 1], (int)b[4 * l + 2], (int)b[4 * l + 3], 0, 0, 0, 0};
	v16f acc = {0};
	acc = mfma4<SCALED>(x, y, acc);
	for (int r = 0; r < 16; r++) c[16 * l + r] = acc[r];
}

// `steps` k-steps into one accumulator tile, as a Gram wave runs them: a, b hold steps x 64 lanes x 4 words
template <int SCALED>
__global__ void k_chain(const uint32_t *a, const uint32_t *b, float *c, int steps)
{
	const unsigned l = threadIdx.x;
	v16f acc = {0};
	for (int s = 0; s < steps; s++) {
		const uint32_t *pa = a + (size_t)s * 256 + 4 * l, *pb = b + (size_t)s * 256 + 4 * l;
		v8i x = {(int)pa[0], (int)pa[1], (int)pa[2], (int)pa[3], 0, 0, 0, 0};
		v8i y = {(int)pb[0], (int)pb[1], (int)pb[2], (int)pb[3], 0, 0, 0, 0};
		acc = mfma4<SCALED>(x, y, acc);
	}
	for (int r = 0; r < 16; r++) c[16 * l + r] = acc[r];
}

template <int FP4>
__global__ void k_rate(float *out, int iters)
{
	v8i x = {(int)threadIdx.x, 1, 2, 3, 0, 0, 0, 0}, y = {5, 6, 7, (int)threadIdx.x, 0, 0, 0, 0};
	v16f acc[4] = {};
	v16i iacc[4] = {};
	for (int i = 0; i < iters; i++) {
#pragma unroll
		for (int t = 0; t < 4; t++) {
			if (FP4 == 1)
				acc[t] = mfma4<1>(x, y, acc[t]);
			else if (FP4 == 2)
				acc[t] = mfma4<0>(x, y, acc[t]);
			else
				iacc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4i{x[0], x[1], x[2], x[3]}, v4i{y[0], y[1], y[2], y[3]}, iacc[t], 0, 0, 0);
		}
	}
	float s = 0;
	for (int t = 0; t < 4; t++)
		for (int r = 0; r < 16; r++) s += acc[t][r] + (float)iacc[t][r];
	out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

int main()
{
	uint32_t *d_a, *d_b;
	float *d_c;
	(void)hipMalloc(&d_a, 64 * 16);
	(void)hipMalloc(&d_b, 64 * 16);
	(void)hipMalloc(&d_c, 64 * 16 * 4);
	std::vector<uint32_t> ha(256), hb(256);
	std::vector<float> hc(1024);
	auto run = [&]() {
		(void)hipMemcpy(d_a, ha.data(), 1024, hipMemcpyHostToDevice);
		(void)hipMemcpy(d_b, hb.data(), 1024, hipMemcpyHostToDevice);
		hipLaunchKernelGGL(k_one<1>, dim3(1), dim3(64), 0, 0, d_a, d_b, d_c);
		(void)hipMemcpy(hc.data(), d_c, 4096, hipMemcpyDeviceToHost);
	};
	// 0. the two forms of the instruction on the same operands, accumulators compared bit for bit.  The Gram steps feed it the
	//    codes 0001, 0010, 0100 and zero only (one bit of a nibble kept by a mask); "any" = all sixteen codes, for the record.
	{
		const int kSteps = 64;
		uint32_t *d_sa, *d_sb;
		(void)hipMalloc(&d_sa, kSteps * 1024);
		(void)hipMalloc(&d_sb, kSteps * 1024);
		std::vector<uint32_t> sa(kSteps * 256), sb(kSteps * 256);
		std::vector<float> c_scaled(1024), c_free(1024);
		uint64_t rng = 0x9E3779B97F4A7C15ull;
		auto next = [&]() {
			rng += 0x9E3779B97F4A7C15ull;
			uint64_t z = rng;
			z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
			z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
			return z ^ (z >> 31);
		};
		static const uint32_t gram_codes[4] = {0x0, 0x1, 0x2, 0x4};
		auto word = [&](int fill) { // 0 .. 3: that Gram code in every nibble; 4: random Gram codes; 5: one bit of every nibble (a
			                        // mask of the k-steps on random data); 6: any code
			uint32_t w = 0;
			if (fill == 5) return (uint32_t)next() & (0x11111111u << (next() % 3));
			for (int nb = 0; nb < 8; nb++) {
				const uint32_t code = fill < 4 ? gram_codes[fill] : fill == 4 ? gram_codes[next() & 3] : (uint32_t)(next() & 15);
				w |= code << (4 * nb);
			}
			return w;
		};
		static const char *fill_name[7] = {"all zero", "all 0001", "all 0010", "all 0100", "random of {0, 0001, 0010, 0100}", "one masked bit per nibble", "any code"};
		int total_diff = 0;
		printf("scaled (scales 0x7F7F7F7F) against scale-free (scales 0): accumulator words that differ, of 1024\n");
		for (int fa = 0; fa < 7; fa++)
			for (int fb = 0; fb < 7; fb++) {
				if ((fa == 6) != (fb == 6)) continue;
				for (int steps : {1, kSteps}) {
					for (auto &w : sa) w = word(fa);
					for (auto &w : sb) w = word(fb);
					(void)hipMemcpy(d_sa, sa.data(), kSteps * 1024, hipMemcpyHostToDevice);
					(void)hipMemcpy(d_sb, sb.data(), kSteps * 1024, hipMemcpyHostToDevice);
					hipLaunchKernelGGL(k_chain<1>, dim3(1), dim3(64), 0, 0, d_sa, d_sb, d_c, steps);
					(void)hipMemcpy(c_scaled.data(), d_c, 4096, hipMemcpyDeviceToHost);
					hipLaunchKernelGGL(k_chain<0>, dim3(1), dim3(64), 0, 0, d_sa, d_sb, d_c, steps);
					(void)hipMemcpy(c_free.data(), d_c, 4096, hipMemcpyDeviceToHost);
					const int diff = memcmp(c_scaled.data(), c_free.data(), 4096) == 0 ? 0 : [&] {
						int d = 0;
						for (int i = 0; i < 1024; i++) d += memcmp(&c_scaled[i], &c_free[i], 4) != 0;
						return d;
					}();
					float mx = 0;
					for (int i = 0; i < 1024; i++) mx = c_free[i] > mx ? c_free[i] : mx;
					printf("  A %-32s B %-32s %2d k-step(s): %d differ (largest entry %g)\n", fill_name[fa], fill_name[fb], steps, diff, mx);
					if (fa != 6) total_diff += diff;
				}
			}
		printf("Gram codes: %s\n", total_diff == 0 ? "the two forms agree bit for bit" : "THE TWO FORMS DIFFER");
		(void)hipFree(d_sa);
		(void)hipFree(d_sb);
		if (hipDeviceSynchronize() != hipSuccess) {
			printf("device error\n");
			return 1;
		}
		if (total_diff) return 2;
	}
	// 1. value decoding: A = code in every nibble of row 0's k = 0 entry only; B = 1.0 (0x2) everywhere
	printf("value decoding (A nibble code -> product with 1.0):");
	for (unsigned code = 0; code < 16; code++) {
		std::fill(ha.begin(), ha.end(), 0u);
		std::fill(hb.begin(), hb.end(), 0x22222222u);
		ha[0] = code; // lane 0, register 0, nibble 0
		run();
		float v = 0;
		for (int i = 0; i < 1024; i++)
			if (hc[i] != 0) v = hc[i];
		printf(" %x:%g", code, v);
	}
	printf("\n");
	// 2. A layout: one nibble = 1.0 at (lane, reg, nib); B all ones -> which C row lights up (all columns); and K position
	//    via a B that is 1.0 only at one k for all columns
	auto crow = [&](int *row_out) {
		// C/D layout of the 32x32 f32 result: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
		int row = -1, cnt = 0;
		for (int l = 0; l < 64; l++)
			for (int r = 0; r < 16; r++)
				if (hc[16 * l + r] != 0) {
					cnt++;
					row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
				}
		*row_out = row;
		return cnt;
	};
	printf("A operand: (lane, reg, nibble) -> row, with B = all ones:\n");
	for (int l : {0, 1, 31, 32, 33, 63})
		for (int rg : {0, 3})
			for (int nb : {0, 7}) {
				std::fill(ha.begin(), ha.end(), 0u);
				std::fill(hb.begin(), hb.end(), 0x22222222u);
				ha[4 * l + rg] = 0x2u << (4 * nb);
				run();
				int row, cnt = crow(&row);
				printf("  lane %2d reg %d nib %d -> row %2d (%d nonzero entries)\n", l, rg, nb, row, cnt);
			}
	// 3. K index of (lane, reg, nibble): A(lane la, reg ra, nib na) = 1 and B(lane lb, reg rb, nib nb) = 1 give a nonzero
	//    product iff they share k.  For A at lane 0 / lane 32, scan all B positions of column 0 (lanes 0 and 32).
	printf("K pairing: A position -> the B position (same k) in column 0:\n");
	for (int la : {0, 32})
		for (int ra : {0, 1, 3})
			for (int na : {0, 1, 7}) {
				std::fill(ha.begin(), ha.end(), 0u);
				ha[4 * la + ra] = 0x2u << (4 * na);
				for (int lb : {0, 32})
					for (int rb = 0; rb < 4; rb++)
						for (int nb = 0; nb < 8; nb++) {
							std::fill(hb.begin(), hb.end(), 0u);
							hb[4 * lb + rb] = 0x2u << (4 * nb);
							run();
							bool any = false;
							for (int i = 0; i < 1024; i++)
								if (hc[i] != 0) any = true;
							if (any) printf("  A(lane %2d reg %d nib %d) <-> B(lane %2d reg %d nib %d)\n", la, ra, na, lb, rb, nb);
						}
			}
	// 4. exact accumulation of many small terms: all A = 0.5 (0x1), all B = 0.5: every entry = 64 * 0.25 = 16
	std::fill(ha.begin(), ha.end(), 0x11111111u);
	std::fill(hb.begin(), hb.end(), 0x11111111u);
	run();
	printf("all 0.5 x 0.5 over K = 64: C[0] = %g (expect 16)\n", hc[0]);
	// 5. issue rate
	float *d_o;
	(void)hipMalloc(&d_o, 1024 * 256 * 4);
	hipEvent_t e0, e1;
	(void)hipEventCreate(&e0);
	(void)hipEventCreate(&e1);
	for (int fp4 = 0; fp4 < 3; fp4++) {
		const int iters = 20000;
		for (int rep = 0; rep < 2; rep++) {
			(void)hipEventRecord(e0, 0);
			if (fp4 == 1)
				hipLaunchKernelGGL(k_rate<1>, dim3(1024), dim3(256), 0, 0, d_o, iters);
			else if (fp4 == 2)
				hipLaunchKernelGGL(k_rate<2>, dim3(1024), dim3(256), 0, 0, d_o, iters);
			else
				hipLaunchKernelGGL(k_rate<0>, dim3(1024), dim3(256), 0, 0, d_o, iters);
			(void)hipEventRecord(e1, 0);
			(void)hipEventSynchronize(e1);
			float ms;
			(void)hipEventElapsedTime(&ms, e0, e1);
			// 1024 WGs x 4 waves over 1024 SIMDs: 4 waves per SIMD, each iters * 4 MFMAs
			const double per_mfma_ns = ms * 1e6 / ((double)iters * 4 * 4);
			if (rep) printf("%s: %.2f ns per MFMA per SIMD (%.0f T MAC/s chip-wide)\n", fp4 == 1 ? "fp4 32x32x64 scaled" : fp4 == 2 ? "fp4 32x32x64 scale-free" : "i8  32x32x32", per_mfma_ns,
			                (fp4 ? 65536.0 : 32768.0) / per_mfma_ns * 1024 / 1e3);
		}
	}
	return 0;
}
